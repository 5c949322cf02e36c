"""vit_hip_depuncture_batch alone at the DAB FIC shape (4096 frames x 3096 output symbols, SOFT16, the FIC mask's map):
    python scripts/depuncture_rate.py LABEL [path/to/libvit_hip.so]
One line: 7 windows of 2000 back-to-back calls between two device events after 50 warm-up calls, us per call, their median, the bytes
read plus written over it, and a digest of the output.  To compare two builds of the library, run the two alternately, one process
each, in one session (profiles/depuncture_rate.txt)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
label = sys.argv[1] if len(sys.argv) > 1 else "library"
from viterbidecodercpp_amd import _lib
if len(sys.argv) > 2:
    _lib.LIB_PATH = os.path.abspath(sys.argv[2])
import torch
from viterbidecodercpp_amd import COMMON_CODES, FIC_PROFILE, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, get_decoding_config

code = COMMON_CODES[4]
pc = get_decoding_config("SOFT16", code.R)
table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
mask = np.asarray(FIC_PROFILE.mask()).astype(bool).reshape(-1)
F, n_out, P = 4096, mask.size, int(mask.sum())
assert n_out == 3096, n_out
rng = np.random.default_rng(1)
d_in = torch.from_numpy(rng.integers(-127, 128, (F, P)).astype(np.int16)).cuda()
out = torch.empty((F, n_out // 4, 4), dtype=torch.int16, device="cuda")
for _ in range(50):
    dec.depuncture(d_in, mask, out=out)
torch.cuda.synchronize()
digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
CALLS, REPEATS = 2000, 7
times = []
for _ in range(REPEATS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        dec.depuncture(d_in, mask, out=out)
    b.record()
    torch.cuda.synchronize()
    times.append(a.elapsed_time(b) / CALLS * 1000.0)
byts = F * (P + n_out) * 2 + n_out * 4
med = sorted(times)[len(times) // 2]
print(f"{label} frames {F} n_out {n_out} P {P} int16: us/call " + " ".join(f"{t:.2f}" for t in times) +
      f" | median {med:.2f} us min {min(times):.2f} max {max(times):.2f} | {byts / med / 1e3:.0f} GB/s read+written | sha256 {digest}", flush=True)
