"""Time of one BatchDecoder.rs_decode (in place) against a device-to-device copy of the same bytes, against frames_extract over the same
bytes and against the decode_stream(s) call that produced them, in one run.  CCSDS RS(255,223) in the dual basis at interleave depth 5
behind Voyager K = 7 R = 1/2 SOFT16: the frames of one stream of 2^26 bits at P = 10232, and 64 rows of 8 frames each.  Inputs: (a) clean
frames, (b) the frames of the real chain at 2.5 dB with the share of codewords that needed correction, (c) every codeword with t
errors.  Every figure is the median of `--sets` windows of `--reps` calls between two device events, after warm-up; the decode runs in place, so a
timed call first restores the frames by a copy whose own time, measured the same way, is taken off: those figures are differences of two
medians (the clean input writes nothing and is timed alone).  The decode_stream(s) baseline is the median of 3 windows of reps / 4 calls.

    python scripts/rs_decode_rate.py [--out profiles/rs_decode_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rs_decode_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (CCSDS_ASM, CCSDS_RS_255_223_DUAL, COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config,
                                       ccsds_randomizer, get_decoding_config, rs_encode_numpy)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    conv = COMMON_CODES[2]
    pc = get_decoding_config("SOFT16", conv.R)
    table = ViterbiBranchTable(conv.K, conv.R, conv.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    rs, I, P, drop, W = CCSDS_RS_255_223_DUAL, 5, 10232, 32, 1024
    nI = rs.n * I
    rng = np.random.default_rng(1)
    pad_np = ccsds_randomizer(nI)
    pad = torch.from_numpy(pad_np).to(dec.device)
    mk = np.array([(CCSDS_ASM[0] >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)
    lines = [f"# {torch.cuda.get_device_name(0)}; CCSDS RS(255,223) dual basis, interleave 5, in place, behind Voyager K=7 R=1/2 SOFT16 decoded at "
             f"window {W}; ms per call, device events, median of {args.sets} windows of {args.reps} calls after warm-up (decode_ms: 3 windows of "
             f"{max(args.reps // 4, 2)}); rs_ms of chain2.5dB and t_errors = median(restore copy + decode) - median(restore copy)",
             "# rows  frames/row  codewords  input  corrected_share  failed_share  rs_ms  rs_GB/s  copy_ms  rs/copy  extract_ms  rs/extract  "
             "decode_ms  rs/decode"]
    for rows, per_row in ((1, (1 << 26) // P), (64, 8)):
        # a few distinct codewords, tiled: the decoder's time does not depend on the data of a clean word
        base = rs_encode_numpy(rs, rng.integers(0, 256, size=(16, rs.k * I), dtype=np.uint8), I)
        sent = base[rng.integers(0, 16, size=rows * per_row)].reshape(rows, per_row, nI)
        bits = np.concatenate([np.broadcast_to(mk, (rows, per_row, 32)), np.unpackbits(sent ^ pad_np, axis=2)], axis=2).reshape(rows, -1)
        n_bits = bits.shape[1]
        d_info = torch.from_numpy(np.packbits(bits, axis=1)).to(dec.device)
        clean_sym = dec.encode(d_info, n_bits, tail=True)                       # [rows][n_bits + K-1][R] at exactly high / low
        # the real chain at 2.5 dB: the project's channel on the device (synth's noise), here in torch on the encoder's symbols
        mid, amp = (pc.soft_decision_high + pc.soft_decision_low) / 2, (pc.soft_decision_high - pc.soft_decision_low) / 2
        var = 10 ** (-(2.5 - 10 * np.log10(conv.R) + 3) / 10)
        gen = torch.Generator(device=dec.device).manual_seed(7)
        x = (clean_sym.float() - mid) / amp + torch.randn(clean_sym.shape, generator=gen, device=dec.device) * var ** 0.5
        noisy_sym = torch.clamp(torch.round(x * amp / (1 + var) ** 0.5 + mid), pc.soft_decision_low, pc.soft_decision_high).to(clean_sym.dtype)
        del x

        def chain(sym):
            if rows == 1:
                decode = lambda: dec.decode_stream(sym[0], begin=True, end=True, window=W)
            else:
                pitch = -(-sym.shape[1] // W) * W
                padded = torch.zeros((rows, pitch, conv.R), dtype=sym.dtype, device=sym.device)
                padded[:, :sym.shape[1]] = sym
                decode = lambda: dec.decode_streams(padded, sym.shape[1], begin=True, end=True, window=W)
            out, got_bits = decode()
            assert got_bits == n_bits
            lock = torch.zeros((rows, 4), dtype=torch.int32, device=dec.device)                  # the frames start at bit 0
            outs = dec.frames_extract(out, n_bits, P, 0, lock, marker=CCSDS_ASM[0], marker_bits=32, drop_bits=drop, pad=pad)
            extract = lambda: dec.frames_extract(out, n_bits, P, 0, lock, marker=CCSDS_ASM[0], marker_bits=32, drop_bits=drop, pad=pad, out=outs)
            return decode, extract, outs

        decode, extract, outs = chain(noisy_sym)
        assert int(outs[1].min().item()) == per_row
        real = outs[0].clone()
        clean = torch.from_numpy(sent).to(dec.device)
        worst = sent.copy().reshape(-1, rs.n, I)
        for c in range(I):                                                      # t errors in every codeword, the same places in all
            worst[:, rng.choice(rs.n, size=rs.t, replace=False), c] ^= rng.integers(1, 256, size=rs.t).astype(np.uint8)
        worst = torch.from_numpy(worst.reshape(rows, per_row, nI)).to(dec.device)
        work, status = torch.empty_like(clean), torch.empty((rows, per_row, I), dtype=torch.int32, device=dec.device)
        dst = torch.empty_like(clean)
        copy_ms = median_ms(torch, lambda: dst.copy_(clean), args.reps, args.sets)
        for _ in range(3):
            extract(), decode()
        extract_ms = median_ms(torch, extract, args.reps, args.sets)
        decode_ms = median_ms(torch, decode, max(args.reps // 4, 2), 3)
        for name, src in (("clean", clean), ("chain2.5dB", real), ("t_errors", worst)):
            def call():
                work.copy_(src)                                                 # in place: every call needs the uncorrected frames again
                dec.rs_decode(rs, work, outs[1], I, status=status)
            for _ in range(3):
                call()
            if name == "clean":                                                 # nothing is written: no restore, no subtraction
                rs_ms = median_ms(torch, lambda: dec.rs_decode(rs, work, outs[1], I, status=status), args.reps, args.sets)
            else:
                restore_ms = median_ms(torch, lambda: work.copy_(src), args.reps, args.sets)
                rs_ms = median_ms(torch, call, args.reps, args.sets) - restore_ms        # the last call leaves work decoded
            st = status.cpu().numpy()
            if name != "chain2.5dB":                                            # the chain's share of failures is a result, not a condition
                assert (st == (0 if name == "clean" else rs.t)).all() and np.array_equal(work.cpu().numpy(), sent), name
            lines.append(f"{rows:6d} {per_row:6d} {st.size:9d} {name:>11s} {(st > 0).mean():8.4f} {(st < 0).mean():8.4f} {rs_ms:10.5f} "
                         f"{clean.numel() / rs_ms / 1e6:9.1f} {copy_ms:10.5f} {rs_ms / copy_ms:7.2f} {extract_ms:10.5f} {rs_ms / extract_ms:7.2f} "
                         f"{decode_ms:10.4f} {rs_ms / decode_ms:8.4f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
