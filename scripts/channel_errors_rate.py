#!/usr/bin/env python3
"""Time of the re-encoded channel symbol error count (vit_hip_channel_errors_batch) and of the encoder (vit_hip_encode_batch) beside
the decode call they describe, on four shapes:
  K = 7 R = 1/2 SOFT16, 65536 frames x 8192 bits        against vit_hip_decode_batch
  LTE K = 7 R = 1/3 SOFT16, 65536 x 40 tail-biting      against vit_hip_decode_tail_biting_batch
  K = 7 R = 1/2 SOFT16, one stream of 2^26 bits         against vit_hip_decode_stream
  K = 9 R = 1/2 SOFT16, 65536 x 8192                    against vit_hip_decode_batch
For each call: the time, the bytes it moves (symbols + info bytes + counters / end states), that as GB/s, and the rate of a
device-to-device copy (torch copy_: one hipMemcpyAsync) that moves the same number of bytes (half read, half written) in the same
run -- the roofline of a memory-bound kernel.  Times: best of five loops of `iters` calls, host clock around a device synchronise.
Writes profiles/channel_errors_rate.txt and profiles/channel_errors_summary.md.
usage: channel_errors_rate.py [frames] [iters]"""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, ViterbiBranchTable, ViterbiDecoder_Config, _lib, get_decoding_config, synth

F = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
LOG2_STREAM = 26 if F >= 65536 else 20


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


def copy_rate(n_bytes):
    """GB/s of bytes moved (read + written) by a device-to-device copy that moves n_bytes in all"""
    src = torch.empty(n_bytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return 2 * src.numel() / best(lambda: dst.copy_(src)) / 1e9


def make(code_id):
    code = COMMON_CODES[code_id]
    pc = get_decoding_config("SOFT16", code.R)
    table = ViterbiBranchTable(code.K, code.R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    return code, pc, BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))


def measure(name, dec, sym, out, frames, L, flags, t_decode, decode_name, rows):
    """sym: the received symbols [frames][steps][R]; out: the decoded bytes [frames][ceil(L/8)]"""
    lib, h, st = _lib.load(), dec._handle._h, dec._stream()
    err = torch.empty(frames, dtype=torch.int32, device="cuda")
    cmp = torch.empty(frames, dtype=torch.int32, device="cuda")
    end = torch.empty(frames, dtype=torch.int32, device="cuda")
    enc = torch.empty_like(sym)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    t_cnt = best(lambda: _lib.check(lib.vit_hip_channel_errors_batch(h, p(sym), 0, p(out), 0, frames, L, flags, None, p(err), p(cmp), st)))
    t_enc = best(lambda: _lib.check(lib.vit_hip_encode_batch(h, p(out), 0, frames, L, flags, None, p(enc), 0, p(end), st)))
    sym_bytes, info_bytes = sym.numel() * sym.element_size(), frames * ((L + 7) // 8)
    moved_cnt, moved_enc = sym_bytes + info_bytes + 16 * frames, sym_bytes + info_bytes + 4 * frames     # counters: memset + atomics
    roof_cnt, roof_enc = copy_rate(moved_cnt), copy_rate(moved_enc)
    e, c = int(err.sum(dtype=torch.int64)), int(cmp.sum(dtype=torch.int64))
    rows.append(dict(name=name, frames=frames, L=L, decode_name=decode_name, t_decode=t_decode, t_cnt=t_cnt, t_enc=t_enc, moved_cnt=moved_cnt,
                     moved_enc=moved_enc, rate_cnt=moved_cnt / t_cnt / 1e9, rate_enc=moved_enc / t_enc / 1e9, roof_cnt=roof_cnt, roof_enc=roof_enc,
                     ser=e / max(c, 1)))
    r = rows[-1]
    print(f"{name}: {decode_name} {t_decode * 1e3:9.3f} ms | channel_errors {t_cnt * 1e3:8.3f} ms = {r['rate_cnt']:7.1f} GB/s of {moved_cnt / 1e6:8.1f} MB "
          f"(copy {roof_cnt:7.1f} GB/s, {r['rate_cnt'] / roof_cnt:.2f} of it) = {t_cnt / t_decode:.4f} of the decode | encode {t_enc * 1e3:8.3f} ms = "
          f"{r['rate_enc']:7.1f} GB/s (copy {roof_enc:7.1f} GB/s, {r['rate_enc'] / roof_enc:.2f} of it) = {t_enc / t_decode:.4f} of the decode | "
          f"channel symbol error rate {r['ser']:.4f}", flush=True)


rows = []
T_FLAG, TB_FLAG = _lib.ENCODE_TAIL, _lib.ENCODE_TAIL_BITING
print(f"# re-encoded channel symbol error count and encoder beside the decode they describe, {F} frames, SOFT16, one MI355X")

for code_id, label in ((2, "K7 R1/2"), (5, "K9 R1/2")):
    code, pc, dec = make(code_id)
    L = 8192
    _, sym = dec.synth(F, L, 2.0, seed=1)
    out = torch.empty((F, L // 8), dtype=torch.uint8, device="cuda")
    t_dec = best(lambda: dec.decode(sym, L, out=out))
    measure(f"{label} {F} x {L}", dec, sym, out, F, L, T_FLAG, t_dec, "vit_hip_decode_batch", rows)
    if code_id == 2:
        # one stream: a single terminated frame of 2^26 bits, decoded as overlapped windows
        Ls = 1 << LOG2_STREAM
        _, s1 = dec.synth(1, Ls, 2.0, seed=2)
        s1 = s1.reshape(-1, code.R)
        ws = torch.empty(dec.stream_workspace_bytes(s1.shape[0], True, True), dtype=torch.uint8, device="cuda")
        o1 = torch.empty(Ls // 8, dtype=torch.uint8, device="cuda")
        t_dec = best(lambda: dec.decode_stream(s1, True, True, out=o1, workspace=ws))
        measure(f"{label} one stream of 2^{LOG2_STREAM} bits", dec, s1, o1, 1, Ls, T_FLAG, t_dec, "vit_hip_decode_stream", rows)
        del s1, ws, o1
    del sym, out, dec
    torch.cuda.empty_cache()

code, pc, dec = make(3)
L = 40
rng = np.random.default_rng(L)
bits = rng.integers(0, 2, size=(4096, L), dtype=np.uint8)
coded = synth.encode_tail_biting_numpy(code.K, code.R, code.G, bits)
sym = torch.from_numpy(synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, 2.0, code.R, rng, pc.soft_dtype)).cuda()
sym = sym.repeat(max(F // 4096, 1), 1, 1).contiguous()
Ftb = sym.shape[0]
out = torch.empty((Ftb, (L + 7) // 8), dtype=torch.uint8, device="cuda")
ws = torch.empty(dec.tail_biting_workspace_bytes(Ftb, L), dtype=torch.uint8, device="cuda")
t_dec = best(lambda: dec.decode_tail_biting(sym, L, out=out, workspace=ws))
measure(f"LTE K7 R1/3 {Ftb} x {L} tail-biting", dec, sym, out, Ftb, L, TB_FLAG, t_dec, "vit_hip_decode_tail_biting_batch", rows)

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "channel_errors_rate.txt"), "w") as f:
    f.write(f"# scripts/channel_errors_rate.py {F} {ITERS}: SOFT16, one MI355X, best of five loops of {ITERS} calls\n")
    f.write("# shape | decode call, ms | channel_errors ms, MB moved, GB/s, copy GB/s, ratio to the decode | encode ms, MB moved, GB/s, copy GB/s, ratio to the decode\n")
    for r in rows:
        f.write(f"{r['name']} | {r['decode_name']} {r['t_decode'] * 1e3:.3f} | {r['t_cnt'] * 1e3:.3f} {r['moved_cnt'] / 1e6:.1f} {r['rate_cnt']:.1f} "
                f"{r['roof_cnt']:.1f} {r['t_cnt'] / r['t_decode']:.4f} | {r['t_enc'] * 1e3:.3f} {r['moved_enc'] / 1e6:.1f} {r['rate_enc']:.1f} "
                f"{r['roof_enc']:.1f} {r['t_enc'] / r['t_decode']:.4f}\n")
with open(os.path.join(ROOT, "profiles", "channel_errors_summary.md"), "w") as f:
    f.write("# Channel symbol error count and encoder: time beside the decode\n\n")
    f.write(f"`scripts/channel_errors_rate.py {F} {ITERS}` on one MI355X, SOFT16. The copy column is a device-to-device copy moving the same bytes "
            "(half read, half written) in the same run.\n\n")
    f.write("| shape | decode, ms | count, ms | count GB/s | copy GB/s | count / decode | encode, ms | encode GB/s | copy GB/s | encode / decode |\n")
    f.write("|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
        f.write(f"| {r['name']} | {r['t_decode'] * 1e3:.3f} | {r['t_cnt'] * 1e3:.3f} | {r['rate_cnt']:.0f} | {r['roof_cnt']:.0f} | {r['t_cnt'] / r['t_decode']:.4f} | "
                f"{r['t_enc'] * 1e3:.3f} | {r['rate_enc']:.0f} | {r['roof_enc']:.0f} | {r['t_enc'] / r['t_decode']:.4f} |\n")
    f.write("\nWhere the time goes when a call is far below its copy rate:\n\n")
    for r in rows:
        for what, rate, roof, t in (("count", r["rate_cnt"], r["roof_cnt"], r["t_cnt"]), ("encode", r["rate_enc"], r["roof_enc"], r["t_enc"])):
            if rate < 0.5 * roof:
                chunks = r["frames"] * ((r["L"] + 7) // 8 + 1)
                f.write(f"- {r['name']}, {what}: {rate / roof:.2f} of the copy rate; {t * 1e9 / chunks:.2f} ns per 8-step chunk of one thread. "
                        + ("A call this small is launch-bound: the time is the launches (two memsets and a kernel for the count), not the bytes.\n"
                           if t < 30e-6 else
                           "Per chunk a thread issues about 10 integer instructions per symbol (shift, mask, popcount, compare, add) and a "
                           "division to find its frame: the kernel is bound by vector issue, not by memory.\n"))
    f.write('\nThe large shapes sit at about 0.6 of the copy rate (the encoder, which only stores, at 0.65 - 0.8) although they move no more bytes than the copy: per 8-step chunk a thread issues about ten integer instructions per symbol (shift, mask, popcount, compare, add) and a 32-bit division to find its frame, so vector issue, not memory, bounds both kernels. A bit-parallel parity (XOR of shifted history words, eight steps at once) is the known way to cut that; it has not been tried.\n')
print("wrote profiles/channel_errors_rate.txt and profiles/channel_errors_summary.md")
