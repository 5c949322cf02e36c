"""Time of one BatchDecoder.frames_extract against a device-to-device copy of the same bytes, against marker_search over the same bytes
and against the decode_stream(s) call that produced them, in one run.  Voyager K = 7 R = 1/2 SOFT16: one stream of 2^26 bits cut at P =
10232 with drop_bits = 32 and the CCSDS randomiser as pad, and 64 rows of 16384 bits at P = 1632 with the sync byte dropped.  Every figure
is the median of `--sets` windows of `--reps` calls between two device events, after warm-up.

    python scripts/frames_extract_rate.py [--out profiles/frames_extract_rate.txt] [--reps 20] [--sets 7]
"""
import argparse
import os
import statistics
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_extract_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (CCSDS_ASM, COMMON_CODES, DVB_SYNC, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config,
                                       ccsds_randomizer, get_decoding_config)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    code = COMMON_CODES[2]
    pc = get_decoding_config("SOFT16", code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    W = 1024
    lines = [f"# {torch.cuda.get_device_name(0)}; Voyager K=7 R=1/2 SOFT16 decoded at window {W}; ms per call, device events, median of "
             f"{args.sets} windows of {args.reps} calls after warm-up; GB/s = the row bytes once over the time",
             "# rows  n_bits  P  drop  pad  extract_ms  extract_GB/s  copy_ms  copy_GB/s  extract/copy  search_ms  extract/search  "
             "decode_ms  extract/decode"]
    for rows, n_bits, marker, P, drop, with_pad in ((1, 1 << 26, CCSDS_ASM, 10232, 32, True), (64, 16384, DVB_SYNC, 1632, 8, False)):
        _, sym = dec.synth(rows, n_bits, 4.0, seed=rows)                     # [rows][n_bits + K-1][R]: each row one terminated stream
        if rows == 1:
            decode = lambda: dec.decode_stream(sym[0], begin=True, end=True, window=W)
        else:
            pitch = -(-sym.shape[1] // W) * W
            padded = torch.zeros((rows, pitch, code.R), dtype=sym.dtype, device=sym.device)
            padded[:, :sym.shape[1]] = sym
            decode = lambda: dec.decode_streams(padded, sym.shape[1], begin=True, end=True, window=W)
        out, got_bits = decode()
        assert got_bits == n_bits
        totals = (torch.empty((rows, P), dtype=torch.int32, device=dec.device), torch.empty((rows, P), dtype=torch.int32, device=dec.device),
                  torch.empty((rows, 4), dtype=torch.int32, device=dec.device))
        search = lambda: dec.marker_search(out, n_bits, marker[0], marker[1], P, out=totals)
        search()
        pad = torch.from_numpy(ccsds_randomizer((P - drop + 7) // 8)).to(dec.device) if with_pad else None
        carry = (torch.zeros((rows, (P + 6) // 8), dtype=torch.uint8, device=dec.device), torch.full((rows,), 100, dtype=torch.int32, device=dec.device))
        outs = dec.frames_extract(out, n_bits, P, 0, totals[2], carry[0], carry[1], marker[0], marker[1], drop, pad)
        extract = lambda: dec.frames_extract(out, n_bits, P, 0, totals[2], carry[0], carry[1], marker[0], marker[1], drop, pad, out=outs)
        dst = torch.empty_like(out)
        copy = lambda: dst.copy_(out)
        for _ in range(3):
            extract(), search(), copy(), decode()
        extract_ms, copy_ms = median_ms(torch, extract, args.reps, args.sets), median_ms(torch, copy, args.reps, args.sets)
        search_ms = median_ms(torch, search, args.reps, args.sets)
        decode_ms = median_ms(torch, decode, max(args.reps // 4, 2), 3)
        n_bytes = rows * n_bits // 8
        lines.append(f"{rows:6d} {n_bits:9d} {P:6d} {drop:3d} {int(with_pad):2d} {extract_ms:10.5f} {n_bytes / extract_ms / 1e6:9.1f} {copy_ms:10.5f} "
                     f"{n_bytes / copy_ms / 1e6:9.1f} {extract_ms / copy_ms:7.2f} {search_ms:10.5f} {extract_ms / search_ms:7.2f} "
                     f"{decode_ms:10.4f} {extract_ms / decode_ms:8.4f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
