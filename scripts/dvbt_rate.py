"""Time of BatchDecoder.dvbt_deinterleave (vit_hip_dvbt_deinterleave_batch) against three things in the same run:
  (a) copy: a device-to-device copy of as many bytes as the call reads plus writes;
  (b) torch: the same result from torch index ops with a precomputed map, what a caller does without the call, checked equal to the
      kernel's output before it is timed: the symbols of even and odd parity each through one index_select over an input with a zero
      column behind it (the padded input and both maps are built once, outside the timed call);
  (c) decode: the decode_stream / decode_streams call behind it, on the symbols it wrote.
Shapes: 8k / 64-QAM / 3/4, one row of 256 OFDM symbols; 2k / QPSK / 1/2, 64 rows of 32 symbols.  SOFT16.  The soft bits are random: the
kernel's work does not depend on the values.  Every figure is the median of `--sets` windows of `--reps` calls between two device events,
after warm-up.

    python scripts/dvbt_rate.py [--out profiles/dvbt_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvbt_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (COMMON_CODES, DVBT_MODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, dvbt_steps_per_symbol,
                                       get_decoding_config)
    from viterbidecodercpp_amd.dvbt import _source_index

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    pc = get_decoding_config("SOFT16", 2)
    dec = BatchDecoder(ViterbiBranchTable(7, 2, COMMON_CODES[2].G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    dev = dec.device
    rng = np.random.default_rng(1)
    lines = [f"# {torch.cuda.get_device_name(0)}; vit_hip_dvbt_deinterleave_batch, SOFT16; ms per call, device events, median of {args.sets} windows of "
             f"{args.reps} calls after warm-up; copy = device-to-device copy of the bytes read plus written; torch = the same result from two "
             "index_select calls with precomputed maps; decode = decode_stream(s) on the symbols written",
             "# shape  rows  n_sym  kernel_ms  GB/s  copy_ms  kernel/copy  torch_ms  torch/kernel  decode_ms  kernel/decode"]
    for mode, v, rate, rows, n_sym in (("8k", 6, 2, 1, 256), ("2k", 2, 0, 64, 32)):
        cell, sps = DVBT_MODES[mode].n_max * v, dvbt_steps_per_symbol(mode, v, rate)
        steps = n_sym * sps
        soft = torch.from_numpy(rng.integers(-127, 128, size=(rows, n_sym, cell)).astype(np.int16)).to(dev)
        padded = torch.cat([soft, soft.new_zeros((rows, n_sym, 1))], dim=2)             # the torch ops' input: a zero column behind, built once
        maps = [torch.from_numpy(np.where(s >= 0, s, cell)).to(dev) for s in (_source_index(mode, v, rate, odd) for odd in (0, 1))]
        pitch = -(-steps // 1024) * 1024                                               # decode_streams reads rows at a multiple of its window
        full = torch.zeros((rows, pitch, 2), dtype=torch.int16, device=dev)
        out = full[:, :steps]
        ref = torch.empty((rows, n_sym, 2 * sps), dtype=torch.int16, device=dev)
        n_bytes = soft.numel() * 2 + rows * steps * 4
        buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)

        def kernel():
            return dec.dvbt_deinterleave(soft, mode, v, rate, parity=0, out=full)

        def copy():
            return dst.copy_(buf)

        def torch_fn():
            ref[:, 0::2] = padded[:, 0::2].index_select(2, maps[0])
            ref[:, 1::2] = padded[:, 1::2].index_select(2, maps[1])
            return ref

        if rows == 1:
            def decode():
                return dec.decode_stream(out[0])
        else:
            def decode():
                return dec.decode_streams(full, steps)

        for _ in range(3):
            kernel(), copy(), torch_fn(), decode()
        kernel()
        assert torch.equal(torch_fn().reshape(rows, steps, 2), out), f"{mode}: the torch ops and the kernel differ"
        t = [median_ms(torch, fn, args.reps, args.sets) for fn in (kernel, copy, torch_fn, decode)]
        lines.append(f"{mode}/v{v}/r{rate} {rows:5d} {n_sym:5d} {t[0]:10.5f} {n_bytes / t[0] / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} "
                     f"{t[2] / t[0]:8.2f} {t[3]:10.5f} {t[0] / t[3]:8.4f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
