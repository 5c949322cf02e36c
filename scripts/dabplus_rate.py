"""Time of one BatchDecoder.dabplus_sync and one BatchDecoder.dabplus_au_table at s = 8 against, in the same run, a device-to-device copy
of the bytes each reads, crc_check(DAB_CRC16) over the whole 110 s bytes of the same superframes (the fixed-length kernel on the same
data), rs_decode on the same clean superframes, and the decode call that produces the logical frames (3-A, n = 8: 1536 bits a frame).
Two shapes: one row of 4096 superframes, and 64 rows of 6.  Every figure is the median of `--sets` windows of `--reps` calls between two
device events, after warm-up.

    python scripts/dabplus_rate.py [--out profiles/dabplus_rate.txt] [--reps 20] [--sets 7]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(torch, fn, reps, sets):
    times = []
    for _ in range(sets):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / reps)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dabplus_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (COMMON_CODES, DAB_CRC16, DABPLUS_RS_120_110, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config,
                                       dabplus_superframe_numpy, eep_profile, get_decoding_config)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    conv = COMMON_CODES[4]
    pc = get_decoding_config("SOFT16", conv.R)
    dec = BatchDecoder(ViterbiBranchTable(conv.K, conv.R, conv.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    s, B = 8, 192
    profile = eep_profile("3-A", s)
    assert profile.info_bits == 8 * B
    rng = np.random.default_rng(1)
    formats = [((0, 1), 2, 5), ((1, 1), 3, 6), ((0, 0), 4, 8), ((1, 0), 6, 11)]
    base = []
    for i in range(16):                                            # a few distinct superframes, tiled: no time depends on clean data
        (dac, sbr), n, first = formats[i % 4]
        free = 110 * s - first - 3 * n                             # what is left when every access unit has one byte and its CRC
        sizes = 1 + np.diff(np.concatenate([[0], np.sort(rng.integers(0, free + 1, size=n - 1)), [free]]))
        aus = [rng.integers(0, 256, size=int(L), dtype=np.uint8) for L in sizes]
        assert first + sum(a.size + 2 for a in aus) == 110 * s
        base.append(dabplus_superframe_numpy(aus, dac, sbr, s).reshape(-1))
    base = np.stack(base)
    lines = [f"# {torch.cuda.get_device_name(0)}; dabplus_sync and dabplus_au_table at s = {s}; ms per call, device events, median of {args.sets} "
             f"windows of {args.reps} calls after warm-up; copy = device-to-device copy of the bytes the call reads (sync: 11 bytes a frame); "
             f"crc_check = DAB_CRC16 over the whole {110 * s} bytes of the same superframes; rs_decode on the same clean superframes; decode = the "
             f"decode call that produces the logical frames (3-A n = {s})",
             "# call  rows  superframes/row  call_ms  copy_ms  call/copy  crc_check_ms  call/crc_check  rs_decode_ms  call/rs_decode  decode_ms  call/decode"]
    for rows, per_row in ((1, 4096), (64, 6)):
        sf = torch.from_numpy(base[rng.integers(0, 16, size=rows * per_row)].reshape(rows, per_row, 120 * s)).to(dec.device)
        logical = sf.view(rows, per_row * 5, B)
        totals = tuple(torch.empty(shape, dtype=torch.int32, device=dec.device) for shape in ((rows, 5), (rows, 5), (rows, 4)))
        status = torch.empty((rows, per_row, s), dtype=torch.int32, device=dec.device)
        info, au = torch.empty((rows, per_row), dtype=torch.int32, device=dec.device), torch.empty((rows, per_row, 6, 3), dtype=torch.int32, device=dec.device)
        crc, syn = (torch.empty((rows, per_row), dtype=torch.int32, device=dec.device) for _ in range(2))
        head, data = torch.empty((rows, per_row * 5, 11), dtype=torch.uint8, device=dec.device), torch.empty((rows, per_row, 110 * s), dtype=torch.uint8, device=dec.device)
        sym = torch.zeros((rows * per_row * 5, profile.steps, 4), dtype=dec._soft_dtype, device=dec.device)
        out = torch.empty((rows * per_row * 5, B), dtype=torch.uint8, device=dec.device)
        calls = {
            "sync": lambda: dec.dabplus_sync(logical, out=totals),                                                 # noqa: E731
            "au_table": lambda: dec.dabplus_au_table(sf, s, None, status, out=(info, au)),                         # noqa: E731
            "copy_sync": lambda: head.copy_(logical[..., :11]),                                                    # noqa: E731
            "copy_au": lambda: data.copy_(sf[..., :110 * s]),                                                      # noqa: E731
            "crc": lambda: dec.crc_check(DAB_CRC16, sf, 8 * (110 * s - 2), crc_out=crc, syndrome_out=syn),         # noqa: E731
            "rs": lambda: dec.rs_decode(DABPLUS_RS_120_110, sf, None, s, status=status),                          # noqa: E731
            "decode": lambda: dec.decode(sym, profile.info_bits, out=out),                                         # noqa: E731
        }
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        assert totals[2][:, 0].tolist() == [0] * rows and totals[2][:, 2].tolist() == [0] * rows and not status.any().item()
        assert (info & 3 == 3).all().item() and ((au[..., 2] == 0) | (au[..., 2] == -1)).all().item()
        ms = {k: median_ms(torch, fn, args.reps, args.sets) for k, fn in calls.items()}
        for name, copy in (("sync", "copy_sync"), ("au_table", "copy_au")):
            lines.append(f"{name:>9s} {rows:5d} {per_row:6d} {ms[name]:10.5f} {ms[copy]:10.5f} {ms[name] / ms[copy]:7.2f} {ms['crc']:10.5f} "
                         f"{ms[name] / ms['crc']:7.2f} {ms['rs']:10.5f} {ms[name] / ms['rs']:8.4f} {ms['decode']:10.5f} {ms[name] / ms['decode']:8.4f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
