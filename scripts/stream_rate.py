#!/usr/bin/env python3
"""Rate of overlapped-window decoding of ONE long stream (vit_hip_decode_stream): K = 7 R = 1/2 {109, 79} SOFT16, one stream of
about 2^26 steps, W = 512, 1024, 4096 at the default extension (48 steps each side), and K = 9 R = 1/2 {491, 369} at W = 1024 (64
each side).  Every segment is sized head + n W + tail (one uniform batch, BEGIN set); with `remainder` on the command line each
shape is also run with half a window more, which adds the one-frame launches of the longer last window.
Prints decoded Gbit/s of EMITTED bits and the ratio of the call's time to vit_hip_decode_batch over the same number n of terminated
frames of head + W + tail - (K-1) bits: the plain update + chainback of the same trellis work.
Times: best of five loops of `iters` calls, host clock around a device synchronise.
`only=K:W` keeps one shape and `remainder-only` only its longer variant (for a profiler run of one shape).
usage: stream_rate.py [log2 steps] [iters] [remainder | remainder-only] [only=K:W] > profiles/stream_rate.txt"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, get_decoding_config, synth

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 26
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REMAINDER = "remainder" in sys.argv[3:]
REMAINDER_ONLY = "remainder-only" in sys.argv[3:]
ONLY = [tuple(int(x) for x in a[5:].split(":")) for a in sys.argv[3:] if a.startswith("only=")]


def best(fn):
    fn()
    t = float("inf")
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            fn()
        torch.cuda.synchronize()
        t = min(t, (time.perf_counter() - t0) / ITERS)
    return t


print(f"# one stream of about 2^{LOG2} steps, SOFT16, default extension 8*(K-1) each side, one MI355X")
for code_id, windows in ((2, (512, 1024, 4096)), (5, (1024,))):
    code = COMMON_CODES[code_id]
    windows = [W for W in windows if not ONLY or (code.K, W) in ONLY]
    if not windows:
        continue
    pc = get_decoding_config("SOFT16", code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    K, R = code.K, code.R
    head = tail = 8 * (K - 1)
    # a 2^16-step piece of a noisy stream at 3 dB, repeated: the kernels' time does not depend on the data
    tx, piece = synth.make_frames_numpy(code, pc, 1, (1 << 16) - 8, 3.0, seed=3)
    base = torch.from_numpy(piece[0][:(1 << 16) - 8]).cuda()
    for W in windows:
        n = ((1 << LOG2) - head - tail) // W
        for extra in ((W // 2,) if REMAINDER_ONLY else (0, W // 2) if REMAINDER else (0,)):
            T = head + n * W + tail + extra
            d_sym = base.repeat(T // base.shape[0] + 1, 1)[:T].contiguous()
            ws = torch.empty(dec.stream_workspace_bytes(T, True, False, W, head, tail), dtype=torch.uint8, device="cuda")
            out = torch.empty((T - tail + 7) // 8, dtype=torch.uint8, device="cuda")
            Lf = head + W + tail - (K - 1)
            frames = base.repeat(n * (Lf + K - 1) // base.shape[0] + 1, 1)[:n * (Lf + K - 1)].reshape(n, Lf + K - 1, R).contiguous()
            fout = torch.empty((n, (Lf + 7) // 8), dtype=torch.uint8, device="cuda")
            dec._ws = None
            t_stream = best(lambda: dec.decode_stream(d_sym, True, False, W, head, tail, out=out, workspace=ws))
            t_plain = best(lambda: dec.decode(frames, Lf, out=fout))
            got = np.unpackbits(out[:1024].cpu().numpy())
            errs = int((got != np.unpackbits(tx[0][:1024])).sum())
            print(f"K={K} R=1/{R} W={W:5d} T={T} ({n} windows{', +1 longer last window' if extra else ''}): stream {t_stream * 1e3:8.3f} ms = "
                  f"{(T - tail) / t_stream / 1e9:6.2f} Gbit/s emitted | decode_batch of {n} frames x {Lf} bits {t_plain * 1e3:8.3f} ms | "
                  f"ratio {t_stream / t_plain:.3f} | bit errors in the first 8192 bits at 3 dB: {errs}", flush=True)
            del d_sym, ws, out, frames, fout
            torch.cuda.empty_cache()
