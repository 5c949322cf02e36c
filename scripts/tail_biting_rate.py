#!/usr/bin/env python3
"""Rate of batched tail-biting decoding (vit_hip_decode_tail_biting_batch) on the LTE shape: K = 7, R = 1/3 {91, 117, 121}, 65536
frames of L = 40 and L = 64 info bits (the PDCCH / PBCH size class), SOFT16 and HARD8, default extension (48 steps each side).
Prints decoded info Gbit/s (F * L bits per call) and the ratio of the call's time to the plain update + chainback of the same batch
already extended (n_steps = S_ext, L = L_ext): what the three side passes (gather + fill, end state, window) cost.
Times: best of five loops of `iters` calls, host clock around a device synchronise.
usage: tail_biting_rate.py [frames] [iters] > profiles/tailbiting_rate.txt"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, get_decoding_config, synth

F = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 50


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


code = COMMON_CODES[3]
assert (code.K, code.R) == (7, 3)
print(f"# tail-biting LTE K=7 R=1/3 {list(code.G)}, {F} frames, default extension 8*(K-1) = {8 * (code.K - 1)} each side, one MI355X")
for dt in ("SOFT16", "HARD8"):
    pc = get_decoding_config(dt, code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    dec = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    for L in (40, 64):
        head = tail = 8 * (code.K - 1)
        S_ext, L_ext = head + L + tail, head + L + tail - (code.K - 1)
        rng = np.random.default_rng(L)
        bits = rng.integers(0, 2, size=(4096, L), dtype=np.uint8)
        coded = synth.encode_tail_biting_numpy(code.K, code.R, code.G, bits)
        sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, 2.0, code.R, rng, pc.soft_dtype)
        d_sym = torch.from_numpy(sym).cuda().repeat(F // 4096, 1, 1).contiguous()
        out = torch.empty((F, (L + 7) // 8), dtype=torch.uint8, device="cuda")
        ws_tb = torch.empty(dec.tail_biting_workspace_bytes(F, L), dtype=torch.uint8, device="cuda")
        ext = d_sym[:, (torch.arange(S_ext, device="cuda") - head) % L].contiguous()
        ext_out = torch.empty((F, (L_ext + 7) // 8), dtype=torch.uint8, device="cuda")
        ws = dec.new_workspace(F, L_ext)
        t_tb = best(lambda: dec.decode_tail_biting(d_sym, L, out=out, workspace=ws_tb))
        t_plain = best(lambda: (dec.update(ext, L_ext, n_steps=S_ext, want_metrics=False, workspace=ws),
                                dec.chainback(F, L_ext, out=ext_out, workspace=ws)))
        fer = float((np.unpackbits(out[:4096].cpu().numpy(), axis=1)[:, :L] != bits).any(axis=1).mean())
        print(f"{dt:6s} L={L:3d} S_ext={S_ext}: tail-biting {t_tb * 1e3:7.3f} ms = {F * L / t_tb / 1e9:6.2f} Gbit/s decoded | "
              f"update+chainback of the extended batch {t_plain * 1e3:7.3f} ms | ratio {t_tb / t_plain:.3f} | FER at 2 dB {fer:.4f}",
              flush=True)
