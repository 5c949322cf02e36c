"""Time of BatchDecoder.is95_deinterleave (vit_hip_is95_deinterleave_batch) and of the chain around it, in one run:
  (a) kernel: the de-interleave call, four outputs, one mask per frame; and kernel_device: the same call captured `--reps` times into one
      graph and replayed, per call -- no Python and no launch path between two kernels, so what is left is the device's time;
  (b) copy: a device-to-device copy of as many bytes as the call reads plus writes;
  (c) torch: the same result from torch index ops with a precomputed map, what a caller does without the call, checked equal to the
      kernel's output before it is timed: the mask unpacked to +-1 and multiplied in, one index_select by the inverse permutation, and
      for every hypothesis view(frames, -1, 2^h).sum(2) and a clamp (the map and the bit shifts are built once, outside the timed call);
  (d) decode: the four decode calls behind it, on the symbols it wrote;
  (e) decide: the rate decision call;
  (f) push: the whole Is95TrafficDecoder.push -- de-interleave, 4 decodes, 2 CRCs, the error counts, the decision -- eager and as one
      captured graph replayed.
Shapes: 65536 frames (64 Walsh channels x 1024 frames) and 64 frames.  SOFT16, the stock code.  The symbols are random: no kernel's work
depends on the values.  Every figure is the median of `--sets` windows of `--reps` calls between two device events, after warm-up.

    python scripts/is95_rate.py [--out profiles/is95_rate.txt] [--reps 20] [--sets 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "is95_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (COMMON_CODES, IS95_RATE_SET_1, BatchDecoder, Is95TrafficDecoder, ViterbiBranchTable, ViterbiDecoder_Config,
                                       get_decoding_config, is95_permutation)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    code = COMMON_CODES[5]
    pc = get_decoding_config("SOFT16", 2)
    dec = BatchDecoder(ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    dev = dec.device
    rng = np.random.default_rng(1)
    lines = [f"# {torch.cuda.get_device_name(0)}; vit_hip_is95_deinterleave_batch and the chain around it, SOFT16, {code.name}; ms per call, device "
             f"events, median of {args.sets} windows of {args.reps} calls after warm-up; copy = device-to-device copy of the bytes the de-interleave "
             "reads plus writes; kernel_device = the call captured reps times into one graph, per call; GB/s_device from it; torch = the same four outputs from torch index ops with a precomputed map; decode = the four decode calls on "
             "the symbols written; decide = the rate decision; push = all nine calls, eager and as one replayed graph",
             "# frames  kernel_ms  kernel_device_ms  GB/s_device  copy_ms  kernel/copy  torch_ms  torch/kernel  decode4_ms  kernel/decode4  decide_ms  push_eager_ms  push_graph_ms"]
    inverse = np.empty(384, dtype=np.int64)
    inverse[is95_permutation()] = np.arange(384)
    d_inverse = torch.from_numpy(inverse).to(dev)
    shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=dev)
    for frames in (65536, 64):
        soft = torch.from_numpy(rng.integers(-127, 128, size=(frames, 384)).astype(np.int16)).to(dev)
        mask = torch.from_numpy(rng.integers(0, 256, size=(frames, 48), dtype=np.uint8)).to(dev)
        out = tuple(torch.empty((frames, r.steps, 2), dtype=torch.int16, device=dev) for r in IS95_RATE_SET_1)
        n_bytes = soft.numel() * 2 + mask.numel() + sum(o.numel() * 2 for o in out)
        buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        rx = Is95TrafficDecoder(dec)
        result = (torch.empty((frames, 4), dtype=torch.int32, device=dev), torch.empty((frames, 22), dtype=torch.uint8, device=dev))

        def kernel():
            return dec.is95_deinterleave(soft, scramble=mask, out=out)

        def copy():
            return dst.copy_(buf)

        def torch_fn():
            sign = 1 - 2 * ((mask.unsqueeze(2) >> shifts) & 1).reshape(frames, 384).to(torch.int32)
            s = (soft.to(torch.int32) * sign).index_select(1, d_inverse)
            return [s.view(frames, -1, r.repeat).sum(2).clamp(pc.soft_decision_low, pc.soft_decision_high).to(torch.int16) for r in IS95_RATE_SET_1]

        def push():
            return rx.push(soft, mask, out=result)

        push()                                                      # allocates the receiver's buffers and workspaces
        sym, dbytes, ws, counts, syndrome = rx._buffers(frames)

        def decode():
            for h, r in enumerate(IS95_RATE_SET_1):
                dec.decode(sym[h], r.L, out=dbytes[h])

        def decide():
            return dec.is95_rate_decide(dbytes, [c[0] for c in counts], [c[1] for c in counts], syndrome, rx.max_ser[0], rx.max_ser[1], out=result)

        for _ in range(3):
            kernel(), copy(), torch_fn(), decode(), decide(), push()
        kernel()
        for got, want in zip(torch_fn(), out):
            assert torch.equal(got.view_as(want), want), f"{frames}: the torch ops and the kernel differ"
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                push()
        torch.cuda.current_stream().wait_stream(stream)
        graph.replay()
        many = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(many, stream=stream):
                for _ in range(args.reps):
                    kernel()
        torch.cuda.current_stream().wait_stream(stream)
        many.replay()
        device_ms = median_ms(torch, many.replay, 5, args.sets) / args.reps
        t = [median_ms(torch, fn, args.reps, args.sets) for fn in (kernel, copy, torch_fn, decode, decide, push, graph.replay)]
        lines.append(f"{frames:7d} {t[0]:10.5f} {device_ms:10.5f} {n_bytes / device_ms / 1e6:9.1f} {t[1]:10.5f} {t[0] / t[1]:7.2f} {t[2]:10.5f} {t[2] / t[0]:8.2f} {t[3]:10.5f} "
                     f"{t[0] / t[3]:8.4f} {t[4]:10.5f} {t[5]:10.5f} {t[6]:10.5f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
