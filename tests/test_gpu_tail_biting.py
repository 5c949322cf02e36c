"""Batched tail-biting decoding (vit_hip_decode_tail_biting_batch) against its restatement on the CPU checker
(tests/tb_reference.py): bytes, end states and tail-biting flags bit for bit on every plan, argument errors, concurrency, graph
capture and the cost of the side passes."""
import ctypes as C
import time

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, Code, _lib
from tests.helpers import DECODE_TYPES, default_ebn0, make_table_config, oracle_cfg
from tests.tb_reference import tb_frames, tb_reference

pytestmark = pytest.mark.gpu


def _no_compiler(monkeypatch, tmp_path):
    """as tests/test_gpu_generic.py: no hipcc and an empty user cache, so a code outside the stock table runs the GENERIC kernels"""
    monkeypatch.setenv("VIT_HIP_HIPCC", "/nonexistent/hipcc")
    monkeypatch.setenv("VIT_HIP_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("VIT_HIP_JIT", raising=False)


def extension_cases(K):
    """(L, head, tail): default extension at L = K, 40, 41, 1000; the least extension; odd lengths; head > L (the extension wraps
    round the frame several times)"""
    return [(K, None, None), (40, None, None), (41, None, None), (1000, None, None), (41, K - 1, K - 1),
            (40, max(13, K - 1), max(19, K - 1)), (K + 1, 3 * (K + 1) + 5, K - 1)]


def decode_and_compare(oracle, code, decode_type, F, L, head=None, tail=None, plan=None, seed=1, dec=None, ebn0="default"):
    import torch

    pc, table, config = make_table_config(code, decode_type)
    ebn0 = default_ebn0(code, decode_type) if ebn0 == "default" else ebn0
    bits, sym = tb_frames(code, pc, F, L, ebn0, seed)
    if dec is None:
        dec = BatchDecoder(table, config) if plan is None else BatchDecoder(table, config, plan=plan)
    out, ends, ok = dec.decode_tail_biting(torch.from_numpy(sym).cuda(), L, head, tail, end_state_out=True, ok_out=True)
    torch.cuda.synchronize()
    want_out, want_ends, want_ok = tb_reference(oracle, code, oracle_cfg(decode_type, code.R), sym, L, head, tail)
    tag = (code.name, decode_type, F, L, head, tail, _lib.PLAN_NAMES[dec.plan])
    got = out.cpu().numpy()
    bad = np.argwhere(got != want_out)
    assert bad.size == 0, f"{tag}: bytes differ first at (frame, byte) = {bad[0]} of {len(bad)}"
    assert np.array_equal(ends.cpu().numpy().view(np.uint32), want_ends), f"{tag}: end states differ"
    assert np.array_equal(ok.cpu().numpy(), want_ok), f"{tag}: tail-biting flags differ"
    return dec, bits, got, want_ok


STOCK_SETS = [(COMMON_CODES[i], t) for i in (2, 3, 4) for t in DECODE_TYPES] + [
    (COMMON_CODES[0], "SOFT16"), (COMMON_CODES[1], "HARD8"), (COMMON_CODES[5], "SOFT16"), (COMMON_CODES[6], "SOFT8")]


@pytest.mark.parametrize("code,decode_type", STOCK_SETS, ids=lambda x: getattr(x, "name", x))
def test_stock_codes_bit_exact(oracle, code, decode_type):
    F = 150 if code.K < 7 else 130 if code.K == 7 else 70       # partial tiles and frame pairs
    dec = None
    for k, (L, head, tail) in enumerate(extension_cases(code.K)):
        dec, _, _, _ = decode_and_compare(oracle, code, decode_type, F, L, head, tail, seed=10 * k + code.K, dec=dec)
    assert dec.plan == _lib.PLAN_REG


@pytest.mark.parametrize("decode_type", DECODE_TYPES)
def test_cassini_bit_exact(oracle, decode_type):
    code = COMMON_CODES[7]
    dec = None
    for k, (L, head, tail) in enumerate([(15, None, None), (41, None, None), (40, 14, 14), (16, 53, 14)]):
        dec, _, _, _ = decode_and_compare(oracle, code, decode_type, 3, L, head, tail, seed=k, dec=dec)
    assert dec.plan == _lib.PLAN_LDS2


@pytest.mark.parametrize("code", [Code("K10", 10, 2, (0o1473, 0o1051)), Code("K11", 11, 2, (0o2565, 0o3043))], ids=lambda c: c.name)
def test_lds2_codes_bit_exact(oracle, code):
    for k, (L, head, tail) in enumerate(extension_cases(code.K)):      # 7 frames: a partial frame pair
        dec, _, _, _ = decode_and_compare(oracle, code, "SOFT16" if k % 2 else "HARD8", 7, L, head, tail, seed=k)
        assert dec.plan == _lib.PLAN_LDS2


@pytest.mark.parametrize("code,decode_type", [(Code("K6", 6, 2, (0o65, 0o57)), "SOFT16"), (COMMON_CODES[3], "SOFT8")],
                         ids=["K6", "LTE"])
def test_plan_lds_bit_exact(oracle, code, decode_type):
    dec = None
    for k, (L, head, tail) in enumerate(extension_cases(code.K)):
        dec, _, _, _ = decode_and_compare(oracle, code, decode_type, 70, L, head, tail, plan=_lib.PLAN_LDS, seed=k, dec=dec)
    assert dec.plan == _lib.PLAN_LDS


def test_generic_kernels_bit_exact(oracle, monkeypatch, tmp_path):
    _no_compiler(monkeypatch, tmp_path)
    code = Code("custom K7", 7, 2, (0o147, 0o135))
    dec = None
    for k, (L, head, tail) in enumerate(extension_cases(code.K)):
        dec, _, _, _ = decode_and_compare(oracle, code, "SOFT16", 130, L, head, tail, seed=k, dec=dec)
    assert dec.plan == _lib.PLAN_REG and "GENERIC" in dec.plan_note, dec.plan_note


# Cassini SOFT8 is bit-exact above but not exact noise-free: tests/test_tail_biting_cpu.py NOISE_FREE_EXACT
@pytest.mark.parametrize("code,decode_type", [(c, t) for c in COMMON_CODES for t in DECODE_TYPES if not (c.K == 15 and t == "SOFT8")],
                         ids=lambda x: getattr(x, "name", x))
def test_noise_free_round_trip(oracle, code, decode_type):
    F = 4 if code.K == 15 else 70
    _, bits, got, ok = decode_and_compare(oracle, code, decode_type, F, 40, ebn0=None, seed=code.K + code.R)
    assert np.array_equal(np.unpackbits(got, axis=1)[:, :40], bits)
    assert np.all(ok == 1)


def test_argument_and_workspace_errors():
    import torch

    code = COMMON_CODES[3]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    lib, h = _lib.load(), dec._handle._h
    F, L = 70, 40
    sym = torch.zeros((F, L, code.R), dtype=torch.int16, device="cuda")
    need = lib.vit_hip_tail_biting_workspace_bytes(h, F, L, 48, 48)
    assert need > 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    out = torch.full((F, 5), 0xAB, dtype=torch.uint8, device="cuda")
    ends = torch.full((F,), 12345, dtype=torch.int32, device="cuda")
    ok = torch.full((F,), 0x77, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731

    def call(symbols=p(sym), frames=F, L=L, head=48, tail=48, workspace=p(ws), nbytes=need, out_ptr=p(out)):
        return lib.vit_hip_decode_tail_biting_batch(h, symbols, frames, L, head, tail, workspace, nbytes, out_ptr, p(ends), p(ok),
                                                    None)

    for kwargs in (dict(L=6), dict(head=5), dict(tail=5), dict(L=6, head=0, tail=0), dict(symbols=None), dict(workspace=None),
                   dict(out_ptr=None)):
        assert call(**kwargs) == _lib.ERR_INVALID_ARG, kwargs
    for L_, hd, tl in ((6, 48, 48), (40, 5, 48), (40, 48, 5)):
        assert lib.vit_hip_tail_biting_workspace_bytes(h, F, L_, hd, tl) == 0
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(workspace=C.c_void_p(ws.data_ptr() + 16)) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.all(out == 0xAB) and torch.all(ends == 12345) and torch.all(ok == 0x77), "a rejected call wrote its outputs"
    with pytest.raises(ValueError):
        dec.decode_tail_biting(sym, L, head=3)
    assert call() == _lib.OK                                                  # the same buffers are fine
    torch.cuda.synchronize()


def test_two_streams_and_graph_capture(oracle):
    import torch

    code = COMMON_CODES[3]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    F, L = 130, 40
    _, sym = tb_frames(code, pc, F, L, 1.5, seed=77)
    d_sym = torch.from_numpy(sym).cuda()
    whole, whole_ends, whole_ok = dec.decode_tail_biting(d_sym, L, end_state_out=True, ok_out=True)
    torch.cuda.synchronize()
    # two calls on two streams, each with its own workspace
    halves = [(0, 64), (64, F)]
    outs = [torch.empty((b - a, 5), dtype=torch.uint8, device="cuda") for a, b in halves]
    ends = [torch.empty(b - a, dtype=torch.int32, device="cuda") for a, b in halves]
    wss = [torch.empty(dec.tail_biting_workspace_bytes(b - a, L), dtype=torch.uint8, device="cuda") for a, b in halves]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for (a, b), o, e, w, s in zip(halves, outs, ends, wss, streams):
        with torch.cuda.stream(s):
            dec.decode_tail_biting(d_sym[a:b], L, out=o, end_state_out=e, ok_out=True, workspace=w)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(outs), whole) and torch.equal(torch.cat(ends), whole_ends)
    # one call captured into a graph on a single stream, replayed on new symbols
    out = torch.empty((F, 5), dtype=torch.uint8, device="cuda")
    e = torch.empty(F, dtype=torch.int32, device="cuda")
    ok = torch.empty(F, dtype=torch.uint8, device="cuda")
    ws = torch.empty(dec.tail_biting_workspace_bytes(F, L), dtype=torch.uint8, device="cuda")
    dec.decode_tail_biting(d_sym, L, out=out, end_state_out=e, ok_out=ok, workspace=ws)    # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec.decode_tail_biting(d_sym, L, out=out, end_state_out=e, ok_out=ok, workspace=ws)
    for seed in (78, 79):
        _, sym = tb_frames(code, pc, F, L, 1.5, seed=seed)
        d_sym.copy_(torch.from_numpy(sym))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_out, want_ends, want_ok = tb_reference(oracle, code, oracle_cfg("SOFT16", code.R), sym, L)
        assert np.array_equal(out.cpu().numpy(), want_out)
        assert np.array_equal(e.cpu().numpy().view(np.uint32), want_ends)
        assert np.array_equal(ok.cpu().numpy(), want_ok)


def _best_of_three(fn, iters=20):
    import torch

    best = float("inf")
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / iters)
    return best


# Measured on one MI355X (profiles/tailbiting_rate.txt): 1.53 -- 1.54 at this shape, not the 1.25 first proposed.  The kernel-time
# split (profiles/tailbiting_kernel_stats.csv) says where it goes against 69 us update + 22 us chainback: the RESUMED update kernel
# the call shares with vit_hip_update_batch_resume runs 85 us (it reads the start metrics and enters at a run-time step), the gather
# of the 53 MB extension 31 us, the end-state and window passes 4.8 us each (one launch apiece, at the launch floor).  The bound
# keeps 14 % above the measurement: a side pass that regresses fails here.
OVERHEAD_BOUND = 1.75


def test_side_pass_overhead():
    """LTE SOFT16, 65536 frames of 40 bits: the whole tail-biting call against the plain update + chainback of the same batch
    already extended (n_steps = S_ext, L = L_ext) -- what the gather, end-state and window passes and the resumed update add"""
    import torch

    code = COMMON_CODES[3]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    F, L = 65536, 40
    head = tail = 8 * (code.K - 1)
    S_ext, L_ext = head + L + tail, head + L + tail - (code.K - 1)
    _, sym = tb_frames(code, pc, 4096, L, 2.0, seed=5)
    d_sym = torch.from_numpy(sym).cuda().repeat(F // 4096, 1, 1).contiguous()
    idx = (torch.arange(S_ext, device="cuda") - head) % L
    ext = d_sym[:, idx].contiguous()
    out = torch.empty((F, 5), dtype=torch.uint8, device="cuda")
    ext_out = torch.empty((F, (L_ext + 7) // 8), dtype=torch.uint8, device="cuda")
    ws_tb = torch.empty(dec.tail_biting_workspace_bytes(F, L), dtype=torch.uint8, device="cuda")
    ws = dec.new_workspace(F, L_ext)

    def tail_biting():
        dec.decode_tail_biting(d_sym, L, out=out, workspace=ws_tb)

    def plain():
        dec.update(ext, L_ext, n_steps=S_ext, want_metrics=False, workspace=ws)
        dec.chainback(F, L_ext, out=ext_out, workspace=ws)

    tail_biting(), plain()
    t_tb, t_plain = _best_of_three(tail_biting), _best_of_three(plain)
    print(f"tail-biting {t_tb * 1e3:.3f} ms, update + chainback of the extended batch {t_plain * 1e3:.3f} ms, "
          f"ratio {t_tb / t_plain:.3f}")
    assert t_tb <= OVERHEAD_BOUND * t_plain, (t_tb, t_plain)
