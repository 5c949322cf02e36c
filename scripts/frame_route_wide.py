#!/usr/bin/env python3
"""Single-frame latency of the header-level drop-in at K = 8 and 9: ONE decoder object, reset -> update -> chainback
(ViterbiDecoder_HIP.update / ViterbiDecoder_Core.chainback over the frame route), 4096 and 8192 bits, the median of 20 calls after
warm-up -- under HOST_ROUTE_AUTO (the wide single-frame kernels, csrc/kernels_one.hpp) and under HOST_ROUTE_LDS (the general LDS plan
on one frame, what this route ran before) in the same process, and, where oracle/_ref is present, the reference's scalar decoder on
one core of the same box.  The per-step slope is (t(8192) - t(4096)) / 4096.  Writes profiles/frame_route_wide.txt (--out)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import pyoracle
from viterbidecodercpp_amd import (COMMON_CODES, Code, ViterbiBranchTable, ViterbiDecoder_Config, ViterbiDecoder_Core, ViterbiDecoder_HIP,
                                   _lib, get_decoding_config, synth)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_route_wide.txt"))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=4)
args = ap.parse_args()

CASES = [(5, COMMON_CODES[5], "SOFT16"), (5, COMMON_CODES[5], "SOFT8"), (5, COMMON_CODES[5], "HARD8"), (6, COMMON_CODES[6], "SOFT16"),
         (None, Code("K8 R2", 8, 2, (0o247, 0o371)), "SOFT16")]
LENGTHS = (4096, 8192)
DT = {"SOFT16": pyoracle.SOFT16, "SOFT8": pyoracle.SOFT8, "HARD8": pyoracle.HARD8}

pyoracle.ensure_built()
oracle = pyoracle.Oracle()
ref = pyoracle.RefLib() if pyoracle.RefLib.available() else None


def median_call(vitdec, flat, L, want):
    times = []
    for rep in range(args.warmup + args.calls):
        vitdec.reset()
        t0 = time.perf_counter()
        ViterbiDecoder_HIP.update(vitdec, flat)
        out = vitdec.chainback(L)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(out, want), "decoded bytes differ from the oracle"
    return float(np.median(times[args.warmup:]))


lines = ["# scripts/frame_route_wide.py: one frame through the drop-in (reset -> update -> chainback on one decoder object), "
         f"median of {args.calls} calls after {args.warmup}, one box",
         "# auto = HOST_ROUTE_AUTO, lds = HOST_ROUTE_LDS (PLAN_LDS on one frame), scalar = the reference's scalar decoder on one core of the same host",
         "# code | type | L | auto ms | lds ms | auto/lds | scalar ms | auto/scalar"]
slopes = []
for code_id, code, decode_type in CASES:
    pc = get_decoding_config(decode_type, code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    vitdec = ViterbiDecoder_Core(table, ViterbiDecoder_Config.from_decoder_config(pc))
    ocfg = pyoracle.stock_config(DT[decode_type], code.R)
    per_len = {}
    for L in LENGTHS:
        _, sym = synth.make_frames_numpy(code, pc, 1, L, 3.0, seed=3)
        flat = sym[0].reshape(-1)
        want = oracle.decode(code.K, code.R, code.G, ocfg, sym[0], L)["bytes"]
        vitdec.set_traceback_length(L)
        t = {}
        for name, route in (("auto", _lib.HOST_ROUTE_AUTO), ("lds", _lib.HOST_ROUTE_LDS)):
            vitdec.set_host_route(route)
            t[name] = median_call(vitdec, flat, L, want)
        vitdec.set_host_route(_lib.HOST_ROUTE_AUTO)
        scalar = None
        if ref is not None and code_id is not None:
            secs, out = ref.bench(code_id, ocfg, sym, 1, L, simd=pyoracle.SCALAR, threads=1, passes=args.calls)
            assert np.array_equal(out[0], want)
            scalar = float(np.median(secs))
        per_len[L] = t
        lines.append(f"{code.name} K={code.K} R={code.R} | {decode_type} | {L} | {t['auto'] * 1e3:.3f} | {t['lds'] * 1e3:.3f} | {t['auto'] / t['lds']:.3f} | "
                     + (f"{scalar * 1e3:.3f} | {t['auto'] / scalar:.3f}" if scalar is not None else "- | -"))
        print(lines[-1], flush=True)
    a, b = LENGTHS
    s_auto = (per_len[b]["auto"] - per_len[a]["auto"]) / (b - a)
    s_lds = (per_len[b]["lds"] - per_len[a]["lds"]) / (b - a)
    slopes.append(f"# {code.name} {decode_type}: {s_auto * 1e9:.0f} ns per trellis step on the wide route, {s_lds * 1e9:.0f} ns on PLAN_LDS ({vitdec.host_route_note()})")
    print(slopes[-1], flush=True)
lines += slopes
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", args.out)
