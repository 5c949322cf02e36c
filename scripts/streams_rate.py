#!/usr/bin/env python3
"""Cost of decoding many lockstep streams in ONE call on one shared window grid (vit_hip_decode_streams): K = 7 R = 1/2 {109, 79}
SOFT16, W = 1024 at the default extension (48 steps each side), `streams` streams of `windows` windows each (T = head + windows W +
tail, the smallest pitch (windows + 1) W, BEGIN set), against
  (a) what one stream per call offers for the same job: `streams` back-to-back vit_hip_decode_stream calls on one HIP stream;
  (b) ONE vit_hip_decode_stream call over a single stream that holds the same streams x windows useful windows.
All three go through the C ABI directly.  Times: best of five loops of `iters` calls, host clock around a device synchronise.
`only` runs the new call alone (for a profiler run of its own).
usage: streams_rate.py [streams] [windows] [iters] [only] > profiles/streams_rate.txt"""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, _lib, get_decoding_config, synth

NS = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ONLY = "only" in sys.argv[4:]


def best(fn, iters):
    fn()
    t = float("inf")
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        t = min(t, (time.perf_counter() - t0) / iters)
    return t


code = COMMON_CODES[2]
pc = get_decoding_config("SOFT16", code.R)
table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
lib, h = _lib.load(), dec._handle._h
K, R, W = code.K, code.R, 1024
head = tail = 8 * (K - 1)
T, pitch, T_one = head + N * W + tail, (N + 1) * W, head + NS * N * W + tail
# a 2^16-step piece of a noisy stream at 3 dB, repeated: the kernels' time does not depend on the data
_, piece = synth.make_frames_numpy(code, pc, 1, (1 << 16) - 8, 3.0, seed=3)
base = torch.from_numpy(piece[0][:(1 << 16) - 8]).cuda()
steps = max(NS * pitch, T_one)
d_sym = base.repeat(steps // base.shape[0] + 1, 1)[:steps].contiguous()
need = (lib.vit_hip_streams_workspace_bytes(h, NS, pitch, T, W, head, tail, 1), lib.vit_hip_stream_workspace_bytes(h, T, W, head, tail, 1),
        lib.vit_hip_stream_workspace_bytes(h, T_one, W, head, tail, 1))
assert min(need) > 0
ws = torch.empty(max(need), dtype=torch.uint8, device="cuda")
nb = (T - tail + 7) // 8
out = torch.empty((NS, nb), dtype=torch.uint8, device="cuda")
out_each = torch.empty((NS, nb), dtype=torch.uint8, device="cuda")
out_one = torch.empty((T_one - tail + 7) // 8, dtype=torch.uint8, device="cuda")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                                     # noqa: E731


def streams():
    assert lib.vit_hip_decode_streams(h, p(d_sym), NS, pitch, T, W, head, tail, 1, p(ws), need[0], p(out), nb, None, st) == 0


def per_call():
    for s in range(NS):
        assert lib.vit_hip_decode_stream(h, p(d_sym, s * pitch * R * 2), T, W, head, tail, 1, p(ws), need[1], p(out_each, s * nb), None, st) == 0


def one_stream():
    assert lib.vit_hip_decode_stream(h, p(d_sym), T_one, W, head, tail, 1, p(ws), need[2], p(out_one), None, st) == 0


print(f"# K=7 R=1/2 SOFT16, W={W}, head=tail={head}, {NS} streams x {N} windows (T={T}, pitch={pitch}), one MI355X")
t_streams = best(streams, ITERS)
print(f"vit_hip_decode_streams, one call, {(NS - 1) * (N + 1) + N} grid windows for {NS * N} useful: {t_streams * 1e3:8.3f} ms = "
      f"{NS * (T - tail) / t_streams / 1e9:6.2f} Gbit/s emitted", flush=True)
if not ONLY:
    t_calls, t_one = best(per_call, max(ITERS // 5, 1)), best(one_stream, ITERS)
    torch.cuda.synchronize()
    assert torch.equal(out, out_each)
    print(f"(a) {NS} vit_hip_decode_stream calls back to back on one HIP stream: {t_calls * 1e3:8.3f} ms | ratio {t_streams / t_calls:.4f}")
    print(f"(b) ONE vit_hip_decode_stream call over one stream of {NS * N} windows (T={T_one}): {t_one * 1e3:8.3f} ms | ratio {t_streams / t_one:.3f}")
