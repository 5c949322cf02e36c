"""Time of one BatchDecoder.crc_check (CRC and syndrome) against a device-to-device copy of the bytes it reads and against the stage in
front of it on the same data, in one run:
  - CCSDS: the frames of one stream of 2^26 bits at P = 10232 (6558 frames) and 64 rows of 8, RS(255,223) dual basis at depth 5, the
    frame check CCSDS_CRC16 over the 8904 data bits of the 1115 bytes in front of the parity; beside rs_decode on the same clean frames;
  - LTE: 65536 blocks of 43 bits (27 payload bits + LTE_CRC16 XOR an RNTI), K = 7 R = 1/3 tail-biting; beside decode_tail_biting on the
    same blocks.
Every figure is the median of `--sets` windows of `--reps` calls between two device events, after warm-up.

    python scripts/crc_rate.py [--out profiles/crc_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (CCSDS_CRC16, CCSDS_RS_255_223_DUAL, COMMON_CODES, LTE_CRC16, BatchDecoder, ViterbiBranchTable,
                                       ViterbiDecoder_Config, crc_append_numpy, get_decoding_config, rs_encode_numpy)

    assert torch.cuda.is_available(), "the measurement needs a GPU"

    def decoder(conv):
        pc = get_decoding_config("SOFT16", conv.R)
        table = ViterbiBranchTable(conv.K, conv.R, conv.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
        return BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))

    rng = np.random.default_rng(1)
    lines = [f"# {torch.cuda.get_device_name(0)}; crc_check with crc and syndrome; ms per call, device events, median of {args.sets} windows of "
             f"{args.reps} calls after warm-up; copy = device-to-device copy of the bytes crc_check reads; before = the stage in front on the same data",
             "# shape  rows  frames/row  data_bits  lanes/frame  crc_ms  crc_GB/s  copy_ms  crc/copy  before  before_ms  crc/before"]

    def row(shape, rows, per_row, n_bits, read_bytes, crc_ms, copy_ms, before, before_ms):
        lanes = 1
        while lanes < 64 and -(-((n_bits + 7) // 8) // lanes) > 16:
            lanes *= 2
        lines.append(f"{shape:>6s} {rows:5d} {per_row:7d} {n_bits:7d} {lanes:4d} {crc_ms:10.5f} {read_bytes / crc_ms / 1e6:9.1f} {copy_ms:10.5f} "
                     f"{crc_ms / copy_ms:7.2f} {before:>20s} {before_ms:10.5f} {crc_ms / before_ms:8.4f}")
        print(lines[-1], flush=True)

    dec = decoder(COMMON_CODES[2])
    rs, I, P = CCSDS_RS_255_223_DUAL, 5, 10232
    data_bits = 8 * (rs.k * I - 2)
    for rows, per_row in ((1, (1 << 26) // P), (64, 8)):
        # a few distinct frames, tiled: neither stage's time depends on the data of a clean frame
        base = rs_encode_numpy(rs, crc_append_numpy(CCSDS_CRC16, rng.integers(0, 256, size=(16, rs.k * I - 2), dtype=np.uint8), data_bits), I)
        frames = torch.from_numpy(base[rng.integers(0, 16, size=rows * per_row)].reshape(rows, per_row, rs.n * I)).to(dec.device)
        status = torch.empty((rows, per_row, I), dtype=torch.int32, device=dec.device)
        crc, syn = (torch.empty((rows, per_row), dtype=torch.int32, device=dec.device) for _ in range(2))
        read = torch.empty((rows, per_row, rs.k * I), dtype=torch.uint8, device=dec.device)
        check = lambda: dec.crc_check(CCSDS_CRC16, frames, data_bits, crc_out=crc, syndrome_out=syn)              # noqa: E731
        decode = lambda: dec.rs_decode(rs, frames, None, I, status=status)                                        # noqa: E731
        copy = lambda: read.copy_(frames[..., :rs.k * I])                                                         # noqa: E731
        for _ in range(3):
            check(), decode(), copy()
        assert not syn.any().item() and not status.any().item()
        row("ccsds", rows, per_row, data_bits, read.numel(), median_ms(torch, check, args.reps, args.sets),
            median_ms(torch, copy, args.reps, args.sets), "rs_decode clean", median_ms(torch, decode, args.reps, args.sets))

    lte = decoder(COMMON_CODES[3])
    F, L = 65536, 43
    rnti = rng.integers(0, 1 << 16, size=F)
    payload = rng.integers(0, 256, size=(F, 4), dtype=np.uint8)
    payload[:, 3] &= 0xE0
    blocks = torch.from_numpy(crc_append_numpy(LTE_CRC16, payload, 27, mask=rnti)).to(lte.device)
    sym = lte.encode(blocks, L, tail=False, tail_biting=True)
    out = lte.decode_tail_biting(sym, L)
    crc, syn = (torch.empty(F, dtype=torch.int32, device=lte.device) for _ in range(2))
    read = torch.empty_like(out)
    check = lambda: lte.crc_check(LTE_CRC16, out, 27, crc_out=crc, syndrome_out=syn)                              # noqa: E731
    decode = lambda: lte.decode_tail_biting(sym, L, out=out)                                                      # noqa: E731
    copy = lambda: read.copy_(out)                                                                                # noqa: E731
    for _ in range(3):
        decode(), check(), copy()
    assert np.array_equal(syn.cpu().numpy().view(np.uint32).astype(np.int64), rnti)
    row("lte", 1, F, 27, read.numel(), median_ms(torch, check, args.reps, args.sets), median_ms(torch, copy, args.reps, args.sets),
        "decode_tail_biting", median_ms(torch, decode, args.reps, args.sets))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
