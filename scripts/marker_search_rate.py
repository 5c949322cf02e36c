"""Time of one BatchDecoder.marker_search against a device-to-device copy of the same bytes and against the decode_stream(s) call that
produced them, in one run.  Voyager K = 7 R = 1/2 SOFT16: one stream of 2^26 bits with the CCSDS marker at P = 10232, and 64 rows of
16384 bits with the DVB-S sync byte at P = 1632.  Timed with device events around work on one stream.

    python scripts/marker_search_rate.py [--out profiles/marker_search_rate.txt] [--reps 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(torch, fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marker_search_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (CCSDS_ASM, COMMON_CODES, DVB_SYNC, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config,
                                       get_decoding_config)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    code = COMMON_CODES[2]
    pc = get_decoding_config("SOFT16", code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    W = 1024
    lines = [f"# {torch.cuda.get_device_name(0)}; Voyager K=7 R=1/2 SOFT16 decoded at window {W}; ms per call, device events, {args.reps} "
             f"repetitions after warm-up",
             "# rows  n_bits  marker_bits  P  search_ms  search_GB/s  copy_ms  copy_GB/s  search/copy  decode_ms  search/decode"]
    for rows, n_bits, marker, P in ((1, 1 << 26, CCSDS_ASM, 10232), (64, 16384, DVB_SYNC, 1632)):
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
        dst = torch.empty_like(out)
        copy = lambda: dst.copy_(out)
        for _ in range(3):
            search(), copy(), decode()
        search_ms, copy_ms = event_ms(torch, search, args.reps), event_ms(torch, copy, args.reps)
        decode_ms = event_ms(torch, decode, max(args.reps // 4, 2))
        n_bytes = rows * n_bits // 8
        lines.append(f"{rows:6d} {n_bits:9d} {marker[1]:4d} {P:6d} {search_ms:10.5f} {n_bytes / search_ms / 1e6:9.1f} {copy_ms:10.5f} "
                     f"{n_bytes / copy_ms / 1e6:9.1f} {search_ms / copy_ms:7.2f} {decode_ms:10.4f} {search_ms / decode_ms:8.4f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
