"""Time of one BatchDecoder.dab_deinterleave (time de-interleaver + depuncturing, one launch) and one BatchDecoder.dab_descramble against,
in the same run:
  (a) copy: a device-to-device copy of as many bytes as the call reads (soft bits, history, map) plus writes (symbols, new history);
  (b) torch: the same result from torch index ops on the device -- sixteen strided slice copies for the delays, then one index_select
      through the map with a zero column --, what a caller writes without the call (checked equal to the kernel's output before it is timed);
  (c) depuncture: vit_hip_depuncture_batch alone on input that is already de-interleaved;
  (d) decode: the decode call behind it, on the symbols it wrote;
and for the dispersal a copy of the bytes read plus written and a torch XOR with a pad.
Shapes: 4096 CIFs of one 3-A n = 8 sub-channel (3072 soft bits in, 6168 symbols out), and 64 rows x 32 CIFs of the same profile (the
price of a launch); the dispersal also on 16 x 4096 frames, where its bytes are the cost; SOFT16; the history is full, so every input frame completes one.
Every figure is the median of `--sets` windows of `--reps` calls between two device events, after warm-up.

    python scripts/dab_rate.py [--out profiles/dab_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dab_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, dab_prbs, eep_profile,
                                       get_decoding_config)
    from viterbidecodercpp_amd.dab import DAB_DELAYS

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    conv = COMMON_CODES[4]
    pc = get_decoding_config("SOFT16", conv.R)
    dec = BatchDecoder(ViterbiBranchTable(conv.K, conv.R, conv.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    dev = dec.device
    rng = np.random.default_rng(1)
    p = eep_profile("3-A", 8)
    n, spf, L, nb = p.n_received, p.symbols_per_frame, p.info_bits, p.info_bits // 8
    idx = torch.from_numpy(p.source_index()).to(dev)
    gather = torch.from_numpy(np.where(p.source_index() >= 0, p.source_index(), n).astype(np.int64)).to(dev)       # column n is the zero column
    mask = p.mask()
    lines = [f"# {torch.cuda.get_device_name(0)}; dab_deinterleave and dab_descramble, SOFT16, profile 3-A n = 8 ({n} soft bits in, {spf} symbols "
             f"out, {L} bits); ms per call, device events, median of {args.sets} windows of {args.reps} calls after warm-up; copy = device-to-device "
             "copy of the bytes read plus written; torch = the same result from torch index ops; depuncture = vit_hip_depuncture_batch alone on "
             "de-interleaved input; decode = decode on the symbols written",
             "# call  rows  cifs  call_ms  GB/s  copy_ms  call/copy  torch_ms  torch/call  depuncture_ms  decode_ms  call/decode"]

    def timed(*fns):
        for _ in range(3):
            for fn in fns:
                fn()
        return [median_ms(torch, fn, args.reps, args.sets) for fn in fns]

    for rows, cifs in ((1, 4096), (64, 32)):
        soft = torch.from_numpy(rng.integers(-127, 128, size=(rows, cifs, n)).astype(np.int16)).to(dev)
        hist = torch.from_numpy(rng.integers(-127, 128, size=(rows, 15 * n)).astype(np.int16)).to(dev)
        fill = torch.full((rows,), 15, dtype=torch.int32, device=dev)
        out = (torch.empty((rows, cifs, spf), dtype=torch.int16, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
               torch.empty((rows, 15 * n), dtype=torch.int16, device=dev), torch.empty(rows, dtype=torch.int32, device=dev))
        sym = out[0]
        deint = torch.empty((rows, cifs, n), dtype=torch.int16, device=dev)

        def fused():
            dec.dab_deinterleave(soft, source_index=idx, hist=hist, fill=fill, out=out)

        def torch_ops():
            S = torch.cat([hist.view(rows, 15, n), soft], dim=1)
            for j, d in enumerate(DAB_DELAYS):
                deint[:, :, j::16] = S[:, d:d + cifs, j::16]
            padded = torch.cat([deint, deint.new_zeros((rows, cifs, 1))], dim=2)
            return padded.index_select(2, gather), S[:, cifs:]

        def depuncture():
            dec.depuncture(deint.view(rows * cifs, n), mask, out=sym2)

        sym2 = torch.empty((rows * cifs, spf // 4, 4), dtype=torch.int16, device=dev)
        decoded = torch.empty((rows * cifs, nb), dtype=torch.uint8, device=dev)

        def decode():
            dec.decode(sym.view(rows * cifs, spf // 4, 4), L, out=decoded)

        n_bytes = soft.numel() * 2 + hist.numel() * 2 + idx.numel() * 4 + sym.numel() * 2 + hist.numel() * 2
        buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        fused()
        want, want_hist = torch_ops()
        torch.cuda.synchronize()
        assert torch.equal(want, sym) and torch.equal(want_hist.reshape(rows, -1), out[2]), "the torch ops and the kernel differ"
        assert out[1].tolist() == [cifs] * rows
        t = timed(fused, lambda: dst.copy_(buf), torch_ops, depuncture, decode)
        lines.append(f"deinterleave {rows:5d} {cifs:5d} {t[0]:10.5f} {n_bytes / t[0] / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} "
                     f"{t[2] / t[0]:8.2f} {t[3]:10.5f} {t[4]:10.5f} {t[0] / t[4]:8.4f}")
        print(lines[-1], flush=True)

        frames = decoded.view(rows, cifs, nb)
        clear = torch.empty_like(frames)
        pad = torch.from_numpy(np.packbits(dab_prbs(L))).to(dev)
        buf2 = torch.empty(2 * frames.numel(), dtype=torch.uint8, device=dev)
        dst2 = torch.empty_like(buf2)
        dec.dab_descramble(frames, L, out=clear)
        torch.cuda.synchronize()
        assert torch.equal(clear, frames ^ pad), "the torch XOR and the kernel differ"
        t = timed(lambda: dec.dab_descramble(frames, L, out=clear), lambda: dst2.copy_(buf2), lambda: torch.bitwise_xor(frames, pad, out=clear))
        lines.append(f"descramble   {rows:5d} {cifs:5d} {t[0]:10.5f} {2 * frames.numel() / t[0] / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} "
                     f"{t[2] / t[0]:8.2f} {'-':>10s} {'-':>10s} {'-':>8s}")
        print(lines[-1], flush=True)
    # the dispersal alone where its bytes, not its launch, are the cost: 65536 frames of the same length
    rows, cifs = 16, 4096
    frames = torch.from_numpy(rng.integers(0, 256, size=(rows, cifs, nb), dtype=np.uint8)).to(dev)
    clear = torch.empty_like(frames)
    pad = torch.from_numpy(np.packbits(dab_prbs(L))).to(dev)
    buf2 = torch.empty(2 * frames.numel(), dtype=torch.uint8, device=dev)
    dst2 = torch.empty_like(buf2)
    dec.dab_descramble(frames, L, out=clear)
    torch.cuda.synchronize()
    assert torch.equal(clear, frames ^ pad), "the torch XOR and the kernel differ"
    t = timed(lambda: dec.dab_descramble(frames, L, out=clear), lambda: dst2.copy_(buf2), lambda: torch.bitwise_xor(frames, pad, out=clear))
    lines.append(f"descramble   {rows:5d} {cifs:5d} {t[0]:10.5f} {2 * frames.numel() / t[0] / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} "
                 f"{t[2] / t[0]:8.2f} {'-':>10s} {'-':>10s} {'-':>8s}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
