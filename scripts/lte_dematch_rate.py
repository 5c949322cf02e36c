"""Time of one BatchDecoder.lte_rate_dematch against three things in the same run:
  (a) copy: a device-to-device copy of as many bytes as the call reads (soft bits, offsets, counts, mask) plus writes;
  (b) decode: the decode_tail_biting call behind it, on the symbols it wrote;
  (c) torch: the same result from torch ops on the device -- per distinct E a descrambling multiply, one index_select and reshape-sum,
      then shift and clamp --, what a caller does without the call (checked equal to the kernel's output before it is timed).
Shapes: 65536 PBCH frames (D = 40, E = 1920, one mask for the batch, shift 4) and 65536 PDCCH candidates (D = 43, E = 72, 144, 288 and 576
from pdcch_candidates over shared control regions of 8 CCEs, one mask bit per region element).
Every figure is the median of `--sets` windows of `--reps` calls between two device events, after warm-up.

    python scripts/lte_dematch_rate.py [--out profiles/lte_dematch_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lte_dematch_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    ap.add_argument("--frames", type=int, default=65536)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, get_decoding_config,
                                       lte_gold_sequence, lte_rate_match_map, pdcch_candidates)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    conv = COMMON_CODES[3]
    pc = get_decoding_config("SOFT16", conv.R)
    dec = BatchDecoder(ViterbiBranchTable(conv.K, conv.R, conv.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    dev, lo, hi = dec.device, pc.soft_decision_low, pc.soft_decision_high
    rng = np.random.default_rng(1)
    F = args.frames
    lines = [f"# {torch.cuda.get_device_name(0)}; lte_rate_dematch, SOFT16; ms per call, device events, median of {args.sets} windows of {args.reps} "
             "calls after warm-up; copy = device-to-device copy of the bytes read plus written; decode = decode_tail_biting on the symbols written; "
             "torch = the same result from torch ops per distinct E",
             "# shape  frames  D  E  dematch_ms  GB/s  copy_ms  dematch/copy  decode_ms  dematch/decode  torch_ms  torch/dematch"]

    def torch_ops(D, E, shift):
        """rows [F_E][E] int16 (descrambled) -> [F_E][3 D] int16 by one index_select and a reshape-sum"""
        n3 = 3 * D
        wraps = -(-E // n3)
        where = np.empty(n3, dtype=np.int64)
        where[lte_rate_match_map(D)] = np.arange(n3)                                   # j of output q
        k = where[None, :] + n3 * np.arange(wraps)[:, None]
        idx = torch.from_numpy(np.where(k < E, k, E).reshape(-1)).to(dev)              # column E is the zero column
        half = (1 << shift) >> 1

        def f(rows):
            padded = torch.cat([rows, rows.new_zeros((rows.shape[0], 1))], dim=1)
            acc = padded.index_select(1, idx).view(rows.shape[0], wraps, n3).sum(dim=1, dtype=torch.int32)
            return ((acc + half) >> shift).clamp_(lo, hi).to(torch.int16)
        return f

    def row(shape, D, E, n_bytes, dematch, sym, torch_fn):
        out = dec.decode_tail_biting(sym, D)
        buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        copy = lambda: dst.copy_(buf)                                                  # noqa: E731
        decode = lambda: dec.decode_tail_biting(sym, D, out=out)                       # noqa: E731
        for _ in range(3):
            dematch(), copy(), decode(), torch_fn()
        assert torch.equal(torch_fn().reshape(-1), sym.reshape(-1)), "the torch ops and the kernel differ"
        t = [median_ms(torch, fn, args.reps, args.sets) for fn in (dematch, copy, decode, torch_fn)]
        lines.append(f"{shape:>6s} {F:7d} {D:4d} {E:>16s} {t[0]:10.5f} {n_bytes / t[0] / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} "
                     f"{t[0] / t[2]:8.4f} {t[3]:10.5f} {t[3] / t[0]:8.2f}")
        print(lines[-1], flush=True)

    # PBCH: [F][1920], one mask for the batch
    D, E, shift = 40, 1920, 4
    soft = torch.from_numpy(rng.integers(-127, 128, size=(F, E)).astype(np.int16)).to(dev)
    packed, bits = lte_gold_sequence(301, E)
    mask = torch.from_numpy(packed).to(dev)
    sign = torch.from_numpy((1 - 2 * bits.astype(np.int16))).to(dev)
    sym = torch.empty((F, D, 3), dtype=torch.int16, device=dev)
    ops = torch_ops(D, E, shift)
    row("pbch", D, str(E), soft.numel() * 2 + mask.numel() + sym.numel() * 2,
        lambda: dec.lte_rate_dematch(soft, D, scramble=mask, scramble_period=E, shift=shift, out=sym), sym, lambda: ops(soft * sign))

    # PDCCH: every aligned candidate of regions of 8 CCEs
    D, shift = 43, 0
    offs, cnts = pdcch_candidates(8)
    regions = -(-F // len(offs))
    region = 8 * 72
    offsets = (np.arange(regions, dtype=np.int64)[:, None] * region + offs[None, :]).reshape(-1)[:F]
    counts = np.tile(cnts, regions)[:F]
    soft = torch.from_numpy(rng.integers(-127, 128, size=regions * region).astype(np.int16)).to(dev)
    bits = rng.integers(0, 2, size=regions * region, dtype=np.uint8)
    mask = torch.from_numpy(np.packbits(bits)).to(dev)
    sign = torch.from_numpy((1 - 2 * bits.astype(np.int16))).to(dev)
    d_off, d_cnt = (torch.from_numpy(x.astype(np.uint32).view(np.int32)).to(dev) for x in (offsets, counts))
    sym = torch.empty((F, D, 3), dtype=torch.int16, device=dev)
    groups = []
    for E in sorted(set(counts.tolist())):
        sel = np.flatnonzero(counts == E)
        at = torch.from_numpy(offsets[sel][:, None] + np.arange(E)[None, :]).to(dev)   # the elements of the candidates of this E
        groups.append((torch.from_numpy(sel).to(dev), at, torch_ops(D, E, shift)))
    ref_out = torch.empty((F, 3 * D), dtype=torch.int16, device=dev)

    def pdcch_torch():
        clean = soft * sign
        for sel, at, ops in groups:
            ref_out[sel] = ops(clean[at])
        return ref_out
    row("pdcch", D, "72,144,288,576", int(counts.sum()) * 2 + int(counts.sum()) // 8 + 8 * F + sym.numel() * 2,
        lambda: dec.lte_rate_dematch(soft, D, E=576, offsets=d_off, counts=d_cnt, scramble=mask, shift=shift, out=sym), sym, pdcch_torch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
