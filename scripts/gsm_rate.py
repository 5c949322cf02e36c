"""Time of the three GSM calls (vit_hip_gsm_deinterleave_batch, vit_hip_gsm_fire_batch, vit_hip_gsm_tchfs_batch) and of the receivers
around them, in one run.  For every item two figures: eager, the call from Python between two device events, and device, the same call
captured `--reps` times into one graph and replayed, per call -- no Python and no launch path between two kernels, so what is left is the
device's time.  Beside every call:
  copy    a device-to-device copy of as many bytes as the call reads plus writes (device figure);
  decode  the decode call behind the de-interleaver (L = 224 in block mode, 185 and 224 in diagonal mode) or in front of the Fire call
          (224) and the TCH/FS call (185) (device figure);
  torch   for the de-interleaver: the same outputs from torch index ops with a precomputed map -- one index_select over the flattened
          bursts of a block, slices for class I and II, a sum over the flag columns --, checked equal to the call's output first.
Items: the de-interleave in block mode and in diagonal mode (with history, all four outputs); the Fire call on clean frames, with a 12-bit
burst in every frame, and on uncorrectable frames; the TCH/FS call; GsmControlDecoder.push and GsmTchfDecoder.push, eager and as a replayed
graph (the TCH/F graph holds two pushes: per push).
Shapes: 65536 blocks (64 rows x 1024) and 64 blocks (64 rows x 1).  SOFT16, GSM_POLYNOMIALS.  Every figure is the median of `--sets`
windows of `--reps` calls after warm-up.

    python scripts/gsm_rate.py [--out profiles/gsm_rate.txt] [--reps 20] [--sets 7]
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


def device_ms(torch, fn, reps, sets, per=1):
    """fn captured reps times into one graph, replayed: ms per call (per: the calls fn itself makes)"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    return median_ms(torch, graph.replay, 5, sets) / reps / per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gsm_rate.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=7)
    args = ap.parse_args()
    import torch

    from viterbidecodercpp_amd import (GSM_BLOCK, GSM_DIAGONAL, GSM_POLYNOMIALS, BatchDecoder, GsmControlDecoder, GsmTchfDecoder, ViterbiBranchTable,
                                       ViterbiDecoder_Config, get_decoding_config, gsm_fire_encode_numpy, gsm_interleave_map)

    assert torch.cuda.is_available(), "the measurement needs a GPU"
    pc = get_decoding_config("SOFT16", 2)
    dec = BatchDecoder(ViterbiBranchTable(5, 2, GSM_POLYNOMIALS, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype),
                       ViterbiDecoder_Config.from_decoder_config(pc))
    dev = dec.device
    rng = np.random.default_rng(1)
    lines = [f"# {torch.cuda.get_device_name(0)}; the GSM calls and the chains around them, SOFT16, polynomials {GSM_POLYNOMIALS} ({dec.plan_note.split(';')[0]}); ms per call, "
             f"device events, median of {args.sets} windows of {args.reps} calls after warm-up; eager = the call from Python; device = the call captured "
             "reps times into one graph, per call; GB/s from device and the bytes read plus written; copy = device-to-device copy of those bytes (device); "
             "decode = the decode call(s) beside it (device); torch = the de-interleaver's outputs from torch index ops with a precomputed map (eager)",
             "# blocks  item                 eager_ms  device_ms     GB/s    copy_ms  device/copy  decode_ms  device/decode   torch_ms  torch/eager"]
    burst, element = gsm_interleave_map(GSM_BLOCK)
    flat = torch.from_numpy((burst.astype(np.int64) * 116 + element)).to(dev)

    def report(blocks, item, eager, device, n_bytes, copy, decode, torch_ms=None):
        tail = "" if torch_ms is None else f" {torch_ms:10.5f} {torch_ms / eager:10.2f}"
        lines.append(f"{blocks:7d}  {item:18s} {eager:10.5f} {device:10.5f} {n_bytes / device / 1e6:8.1f} {copy:10.5f} {device / copy:10.2f} {decode:10.5f} {device / decode:12.4f}" + tail)
        print(lines[-1], flush=True)

    for rows, m in ((64, 1024), (64, 1)):
        n = rows * m
        timed = lambda fn: (median_ms(torch, fn, args.reps, args.sets), device_ms(torch, fn, args.reps, args.sets))
        bursts = torch.from_numpy(rng.integers(-127, 128, size=(rows, 4 * m, 116)).astype(np.int16)).to(dev)
        full, class1 = torch.empty((rows, m, 228, 2), dtype=torch.int16, device=dev), torch.empty((rows, m, 189, 2), dtype=torch.int16, device=dev)
        class2, steal = torch.empty((rows, m, 78), dtype=torch.int16, device=dev), torch.empty((rows, m), dtype=torch.int32, device=dev)
        n_out = torch.empty(rows, dtype=torch.int32, device=dev)
        hist = [torch.zeros((rows, 464), dtype=torch.int16, device=dev) for _ in range(2)]
        fill = [torch.full((rows,), 4, dtype=torch.int32, device=dev) for _ in range(2)]
        b224, b185 = torch.empty((n, 28), dtype=torch.uint8, device=dev), torch.empty((n, 24), dtype=torch.uint8, device=dev)
        outs = {"full": full, "class1": class1, "class2": class2, "steal": steal, "n_out": n_out}

        def copy_ms(n_bytes):
            buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(buf)
            return device_ms(torch, lambda: dst.copy_(buf), args.reps, args.sets)

        def block():
            return dec.gsm_deinterleave(bursts, GSM_BLOCK, out=outs)

        def diagonal():
            return dec.gsm_deinterleave(bursts, GSM_DIAGONAL, hist=hist[0], fill=fill[0], out=dict(outs, hist_out=hist[1], fill_out=fill[1]))

        def torch_block():
            coded = bursts.view(n, 4 * 116).index_select(1, flat)
            return coded, coded[:, :378].contiguous(), coded[:, 378:].contiguous(), bursts.view(n, 4, 116)[:, :, 57:59].sum((1, 2), dtype=torch.int32)

        decode224 = lambda: dec.decode(full.view(n, 228, 2), 224, out=b224)
        decode185 = lambda: dec.decode(class1.view(n, 189, 2), 185, out=b185)
        block()
        for got, want in zip(torch_block(), (full, class1, class2, steal)):
            assert torch.equal(got.reshape(-1), want.reshape(-1)), "the torch ops and the kernel differ"
        d224, d185 = device_ms(torch, decode224, args.reps, args.sets), device_ms(torch, decode185, args.reps, args.sets)
        io = bursts.numel() * 2 + (full.numel() + class1.numel() + class2.numel()) * 2 + steal.numel() * 4
        e, d = timed(block)
        report(n, "deinterleave block", e, d, io, copy_ms(io), d224, median_ms(torch, torch_block, args.reps, args.sets))
        e, d = timed(diagonal)
        report(n, "deinterleave diag", e, d, io + rows * 464 * 4, copy_ms(io + rows * 464 * 4), d224 + d185)

        sent = gsm_fire_encode_numpy(rng.integers(0, 256, size=(n, 23), dtype=np.uint8))
        burst12, noise = sent.copy(), sent.copy()
        burst12[:, 10] ^= 0x0F
        burst12[:, 11] ^= 0xF7                                        # twelve bits from bit 84 on, both ends flipped
        noise[:, 3], noise[:, 20] = noise[:, 3] ^ 0x81, noise[:, 20] ^ 0x42
        status, data = torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty((n, 23), dtype=torch.uint8, device=dev)
        fire_io = n * (28 + 23 + 16)
        fire_copy = copy_ms(fire_io)
        for item, frames, want in (("fire clean", sent, 0), ("fire 12-bit burst", burst12, 12), ("fire uncorrectable", noise, -1)):
            d_frames = torch.from_numpy(frames).to(dev)
            fire = lambda: dec.gsm_fire(d_frames, 12, out=(status, data))
            fire()
            assert (status[:, 0] == want).all(), item
            e, d = timed(fire)
            report(n, item, e, d, fire_io, fire_copy, d224)
        c2 = class2.view(n, 78)
        speech, parity = torch.empty((n, 33), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev)
        tchfs_io = n * (24 + 156 + 33 + 8)
        e, d = timed(lambda: dec.gsm_tchfs(b185, c2, out=(speech, parity)))
        report(n, "tchfs", e, d, tchfs_io, copy_ms(tchfs_io), d185)

        control, traffic = GsmControlDecoder(dec), GsmTchfDecoder(dec)
        c_out = (torch.empty((n, 23), dtype=torch.uint8, device=dev), status)
        t_out = (speech, parity, data, status, steal.view(n))
        push_c = lambda: control.push(bursts, out=c_out)
        push_t = lambda: traffic.push(bursts, out=t_out)
        push_c(), push_t(), push_t()

        def two():
            push_t(), push_t()

        e, d = timed(push_c)
        report(n, "control push", e, d, io, copy_ms(io), d224)
        e, d = median_ms(torch, push_t, args.reps, args.sets), device_ms(torch, two, args.reps, args.sets, per=2)
        report(n, "TCH/F push", e, d, io, copy_ms(io), d224 + d185)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
