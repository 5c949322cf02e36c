"""Batched tail-biting decoding (vit_hip_decode_tail_biting_batch) against its restatement on the CPU checker
(tests/tb_reference.py): bytes, end states and tail-biting flags bit for bit on every plan, argument errors, concurrency, graph
capture and the cost of the side passes."""
import ctypes as C
import time

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, Code, ViterbiBranchTable, ViterbiDecoder_Config, _lib
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


# ---- every K = 2 .. 16, R = 1 .. 8, both widths, every plan family -----------------------------------------------------------
# Polynomial sets from the other suites only, so that nothing is compiled on the GPU host: PLAN_REG at the run-time instantiated sets
# of tests/jit_codes.txt (at the width listed there), GENERIC at the rate-1 sets of test_gpu_generic.py::SETS, PLAN_LDS2 at the sets
# of test_gpu_parity.py::test_lds2_plan_large_k and the K = 16 set of test_gpu_fuzz.py, PLAN_LDS at K = 2, K6 R7 (test_gpu_api.py),
# K7 R8 (test_gpu_latency.py), K15 and K16.
REG, GENERIC, LDS, LDS2 = "REG", "GENERIC", "LDS", "LDS2"
K16 = (46749, 58851)
SWEEP = [
    (2, 2, (0o3, 0o1), "SOFT16", REG), (2, 3, (0o3, 0o2, 0o3), "HARD8", REG),
    (2, 2, (0o3, 0o1), "SOFT16", LDS), (2, 2, (0o3, 0o1), "SOFT8", LDS),
    (3, 4, (0o5, 0o7, 0o7, 0o5), "HARD8", REG), (4, 2, (0o15, 0o17), "SOFT16", REG),
    (5, 5, (0o27, 0o31, 0o33, 0o37, 0o35), "SOFT16", REG), (5, 1, (0o27,), "HARD8", GENERIC),
    (6, 6, (0o65, 0o57, 0o75, 0o53, 0o71, 0o47), "HARD8", REG), (6, 7, (0o65, 0o57, 0o75, 0o53, 0o71, 0o47, 0o77), "SOFT16", LDS),
    (7, 5, (0o171, 0o133, 0o165, 0o117, 0o135), "SOFT8", REG), (7, 6, (0o171, 0o133, 0o165, 0o117, 0o135, 0o157), "SOFT16", REG),
    (7, 1, (0o165,), "SOFT16", GENERIC),
    (7, 8, (0o171, 0o133, 0o165, 0o117, 0o135, 0o157, 0o145, 0o173), "SOFT8", LDS),
    (8, 2, (0o371, 0o247), "SOFT8", REG), (8, 6, (0o371, 0o247, 0o367, 0o331, 0o225, 0o313), "SOFT16", REG),
    (8, 1, (0o371,), "SOFT8", GENERIC),
    (9, 5, (0o557, 0o663, 0o711, 0o561, 0o753), "HARD8", REG), (9, 6, (0o557, 0o663, 0o711, 0o561, 0o753, 0o715), "SOFT16", REG),
    (9, 1, (0o753,), "SOFT16", GENERIC),
    (10, 5, (0o1167, 0o1545, 0o1117, 0o1365, 0o1633), "SOFT16", LDS2),
    (11, 5, (0o3345, 0o3613, 0o2671, 0o3175, 0o2353), "SOFT8", LDS2),
    (11, 6, (0o3345, 0o3613, 0o2671, 0o3175, 0o2353, 0o3661), "HARD8", LDS2),
    (12, 2, (0o4335, 0o5723), "SOFT8", LDS2), (12, 5, (0o4335, 0o5723, 0o6265, 0o7173, 0o5537), "SOFT16", LDS2),
    (12, 6, (0o4335, 0o5723, 0o6265, 0o7173, 0o5537, 0o6747), "HARD8", LDS2),
    (13, 2, (0o10533, 0o17661), "SOFT16", LDS2), (13, 6, (0o10533, 0o10675, 0o17661, 0o13271, 0o15353, 0o16475), "SOFT8", LDS2),
    (14, 2, (0o21645, 0o35661), "SOFT16", LDS2),
    (15, 6, COMMON_CODES[7].G, "SOFT16", LDS),
    (16, 2, K16, "HARD8", LDS2), (16, 2, K16, "SOFT16", LDS),
]
PLAN_OF = {REG: _lib.PLAN_REG, GENERIC: _lib.PLAN_REG, LDS: _lib.PLAN_LDS, LDS2: _lib.PLAN_LDS2}


def sweep_cases(K):
    """(F, L, head, tail): F = 1 and 2, frame counts that leave a partial tile or frame pair; L = K, head > L, heads that are no
    multiple of 8.  K >= 14: a few frames and no L = 1000, as elsewhere in the suite."""
    if K >= 14:
        return [(1, K, None, None), (2, 41, K - 1, K - 1), (3, K + 1, 3 * (K + 1) + 5, K - 1), (2, 40, K + 3, K)]
    Fs = [1, 2, 70, 130, 67, 3, 150] if K <= 9 else [1, 2, 7, 3, 5, 2, 1]
    return [(F,) + c for F, c in zip(Fs, extension_cases(K))]


@pytest.mark.parametrize("K,R,G,decode_type,family", SWEEP, ids=lambda x: x if isinstance(x, (int, str)) else None)
def test_sweep_k_rate_width_plan(oracle, monkeypatch, tmp_path, K, R, G, decode_type, family):
    if family == GENERIC:
        _no_compiler(monkeypatch, tmp_path)
    code = Code(f"K{K}R{R}", K, R, tuple(G))
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config) if family == GENERIC else BatchDecoder(table, config, plan=PLAN_OF[family])
    assert dec.plan == PLAN_OF[family], dec.plan_note
    assert ("GENERIC" in dec.plan_note) == (family == GENERIC), dec.plan_note
    for k, (F, L, head, tail) in enumerate(sweep_cases(K)):
        decode_and_compare(oracle, code, decode_type, F, L, head, tail, seed=100 * K + 10 * R + k, dec=dec)
    assert dec.plan == PLAN_OF[family]


# ---- random decoder configs --------------------------------------------------------------------------------------------------
RANDOM_CASES = [
    (COMMON_CODES[1], REG), (COMMON_CODES[2], REG), (COMMON_CODES[5], REG), (Code("custom K7", 7, 2, (0o147, 0o135)), GENERIC),
    (Code("K2", 2, 2, (0o3, 0o1)), LDS), (Code("K11", 11, 2, (0o3345, 0o3613)), LDS2), (Code("K16", 16, 2, K16), LDS2),
]


@pytest.mark.parametrize("width", [2, 1])
@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_random_configs(oracle, monkeypatch, tmp_path, case, width):
    """any ViterbiDecoder_Config (tests/test_gpu_fuzz.py::random_config: thresholds 0, type-max and random; wrapping error_t
    arithmetic), in-range and full-type-range symbols, random head / tail in [K-1, 3L]: every metric starts at
    initial_start_error and the end state is the unsigned argmin of whatever the arithmetic left"""
    import torch
    from tests.test_gpu_fuzz import random_config

    code, family = RANDOM_CASES[case]
    if family == GENERIC:
        _no_compiler(monkeypatch, tmp_path)
    K, R = code.K, code.R
    rng = np.random.default_rng(7000 + 10 * case + width)
    sdt = np.int16 if width == 2 else np.int8
    lim = 1 << (8 * width - 1)
    for trial in range(4):
        cfg = random_config(rng, width, trial)
        table = ViterbiBranchTable(K, R, code.G, cfg.high, cfg.low, sdt)
        config = ViterbiDecoder_Config(cfg.max_error, cfg.initial_start_error, cfg.initial_non_start_error,
                                       cfg.renormalisation_threshold, np.uint16 if width == 2 else np.uint8)
        dec = BatchDecoder(table, config) if family == GENERIC else BatchDecoder(table, config, plan=PLAN_OF[family])
        assert dec.plan == PLAN_OF[family] and ("GENERIC" in dec.plan_note) == (family == GENERIC), dec.plan_note
        F = int(rng.integers(1, 40)) if K < 11 else int(rng.integers(1, 4))
        L = int(rng.integers(K, 60)) if K < 14 else int(rng.integers(K, 24))
        head, tail = (int(x) for x in rng.integers(K - 1, 3 * L + 1, size=2))
        if trial % 2 == 0:
            sym = rng.integers(cfg.low, cfg.high + 1, size=(F, L, R)).astype(sdt)
        else:
            sym = rng.integers(-lim, lim, size=(F, L, R)).astype(sdt)
        out, ends, ok = dec.decode_tail_biting(torch.from_numpy(sym).cuda(), L, head, tail, end_state_out=True, ok_out=True)
        torch.cuda.synchronize()
        want_out, want_ends, want_ok = tb_reference(oracle, code, cfg, sym, L, head, tail)
        tag = (code.name, family, trial, F, L, head, tail, cfg)
        assert np.array_equal(out.cpu().numpy(), want_out), tag
        assert np.array_equal(ends.cpu().numpy().view(np.uint32), want_ends), tag
        assert np.array_equal(ok.cpu().numpy(), want_ok), tag


# ---- ties in the argmin across lanes and wavefronts ---------------------------------------------------------------------------
def select_groups(K, error_bytes, states):
    """(lanes, wavefronts) of the end-state pass (csrc/kernels_tb.hpp) that hold these states: K <= 9 one lane per VB bytes of a
    frame's metrics, VB = min(16, N * sizeof(error_t)); K >= 10 16-byte chunk c goes to thread c mod 256, wavefront (c mod 256) / 64"""
    N = 1 << (K - 1)
    if K <= 9:
        V = min(16, N * error_bytes) // error_bytes
        return {s // V for s in states}, {0}
    c = [s // (16 // error_bytes) for s in states]
    return set(c), {(x % 256) // 64 for x in c}


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
@pytest.mark.parametrize("code,j", [(COMMON_CODES[3], 5), (COMMON_CODES[5], 6), (Code("K11", 11, 2, (0o2565, 0o3043)), 10),
                                    (Code("K16", 16, 2, K16), 13)], ids=["K7", "K9", "K11", "K16"])
def test_argmin_ties_across_lanes_and_wavefronts(oracle, code, j, decode_type):
    """the last j steps of the extension are erasures (symbol 0: every branch costs the same), so the 2^j states the best state
    reaches over them end on the same minimum -- an aligned block of states (next = (state << 1 | bit) mod N) that spans several
    lanes of the end-state pass, and several wavefronts where the frame's metrics have them.  The lowest state of the block wins."""
    import torch

    K = code.K
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    F = 40 if K <= 9 else 3
    for L, head, tail in ((40, None, None), (K + 1, 2 * K + 3, K + j)):
        hd = 8 * (K - 1) if head is None else head
        tl = 8 * (K - 1) if tail is None else tail
        S_ext = hd + L + tl
        _, sym = tb_frames(code, pc, F, L, default_ebn0(code, decode_type), seed=K + L)
        for i in range(j):
            sym[:, (S_ext - 1 - i - hd) % L] = 0
        out, ends, ok = dec.decode_tail_biting(torch.from_numpy(sym).cuda(), L, head, tail, end_state_out=True, ok_out=True)
        torch.cuda.synchronize()
        want_out, want_ends, want_ok, final = tb_reference(oracle, code, oracle_cfg(decode_type, code.R), sym, L, head, tail,
                                                           want_metrics=True)
        for f in range(F):                                  # the ties are real, and cross the boundaries they are meant to
            tied = np.flatnonzero(final[f] == final[f].min())
            lanes, waves = select_groups(K, pc.error_bytes, tied)
            _, all_waves = select_groups(K, pc.error_bytes, range(1 << (K - 1)))
            assert len(tied) >= 2 and len(lanes) >= 2, (f, tied)
            assert len(waves) >= min(2, len(all_waves)), (f, tied, waves)
        tag = (code.name, decode_type, L, head, tail, _lib.PLAN_NAMES[dec.plan])
        assert np.array_equal(ends.cpu().numpy().view(np.uint32), want_ends), tag
        assert np.array_equal(out.cpu().numpy(), want_out), tag
        assert np.array_equal(ok.cpu().numpy(), want_ok), tag


# ---- outputs and workspace that hold stale bytes ------------------------------------------------------------------------------
POISON_CASES = [(COMMON_CODES[3], "SOFT16", REG), (Code("custom K7", 7, 2, (0o147, 0o135)), "SOFT8", GENERIC),
                (Code("K2", 2, 2, (0o3, 0o1)), "SOFT8", LDS), (Code("K2", 2, 2, (0o3, 0o1)), "SOFT16", LDS),
                (Code("K11", 11, 2, (0o2565, 0o3043)), "HARD8", LDS2)]


@pytest.mark.parametrize("case", range(len(POISON_CASES)))
def test_poisoned_outputs_and_workspace(oracle, monkeypatch, tmp_path, case):
    """workspace, bytes, end states and flags pre-filled with two different patterns: every byte of the result (the pad bits past
    L in each frame's last byte included) is written by the call and equals the reference; then through the C ABI with only the
    end states, only the flags and neither asked for, the same bytes"""
    import torch

    code, decode_type, family = POISON_CASES[case]
    if family == GENERIC:
        _no_compiler(monkeypatch, tmp_path)
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config) if family == GENERIC else BatchDecoder(table, config, plan=PLAN_OF[family])
    assert dec.plan == PLAN_OF[family] and ("GENERIC" in dec.plan_note) == (family == GENERIC), dec.plan_note
    F, L, head, tail = (67, 41, 13, code.K + 2) if code.K < 10 else (5, 41, 13, code.K + 2)
    nb = (L + 7) // 8
    _, sym = tb_frames(code, pc, F, L, default_ebn0(code, decode_type), seed=31 + case)
    d_sym = torch.from_numpy(sym).cuda()
    want_out, want_ends, want_ok = tb_reference(oracle, code, oracle_cfg(decode_type, code.R), sym, L, head, tail)
    need = dec.tail_biting_workspace_bytes(F, L, head, tail)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((F, nb), dtype=torch.uint8, device="cuda")
    ends = torch.empty(F, dtype=torch.int32, device="cuda")
    ok = torch.empty(F, dtype=torch.uint8, device="cuda")
    results = []
    for pattern in (0xFF, 0x5A):
        for t in (ws, out, ok):
            t.fill_(pattern)
        ends.view(torch.uint8).fill_(pattern)
        dec.decode_tail_biting(d_sym, L, head, tail, out=out, end_state_out=ends, ok_out=ok, workspace=ws)
        torch.cuda.synchronize()
        got = (out.cpu().numpy(), ends.cpu().numpy().view(np.uint32), ok.cpu().numpy())
        tag = (code.name, decode_type, family, hex(pattern))
        assert np.array_equal(got[0], want_out), tag
        assert np.array_equal(got[1], want_ends), tag
        assert np.array_equal(got[2], want_ok), tag
        results.append(got)
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    lib, h = _lib.load(), dec._handle._h
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    for with_ends, with_ok in ((True, False), (False, True), (False, False)):
        for t in (ws, out, ok):
            t.fill_(0xC3)
        ends.view(torch.uint8).fill_(0xC3)
        rc = lib.vit_hip_decode_tail_biting_batch(h, p(d_sym), F, L, head, tail, p(ws), need, p(out),
                                                  p(ends) if with_ends else None, p(ok) if with_ok else None, None)
        assert rc == _lib.OK
        torch.cuda.synchronize()
        tag = (code.name, decode_type, family, with_ends, with_ok)
        assert np.array_equal(out.cpu().numpy(), want_out), tag
        if with_ends:
            assert np.array_equal(ends.cpu().numpy().view(np.uint32), want_ends), tag
        else:
            assert torch.all(ends.view(torch.uint8) == 0xC3), tag             # not asked for: not written
        if with_ok:
            assert np.array_equal(ok.cpu().numpy(), want_ok), tag
        else:
            assert torch.all(ok == 0xC3), tag


# ---- batches large enough for the gather's grid-stride loop (8192 blocks of 256 threads, 16 bytes each) ----------------------
def _large_batch_check(oracle, code, decode_type, F, distinct, L, seed):
    import torch

    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    head = tail = 8 * (code.K - 1)
    chunks = -(-F * (head + L + tail) * code.R * pc.soft_bytes // 16)
    assert chunks > 8192 * 256, chunks                        # the gather strides at least once
    _, sym = tb_frames(code, pc, distinct, L, default_ebn0(code, decode_type), seed=seed)
    d_sym = torch.from_numpy(sym).cuda().repeat(F // distinct, 1, 1).contiguous()
    out, ends, ok = dec.decode_tail_biting(d_sym, L, end_state_out=True, ok_out=True)
    torch.cuda.synchronize()
    want_out, want_ends, want_ok = tb_reference(oracle, code, oracle_cfg(decode_type, code.R), sym, L)
    src = np.arange(F) % distinct                              # frame f is a copy of source frame f mod distinct
    got = out.cpu().numpy()
    bad = np.flatnonzero((got != want_out[src]).any(axis=1))
    assert bad.size == 0, f"{code.name}: bytes differ in {bad.size} of {F} frames, first {bad[0]}"
    bad = np.flatnonzero(ends.cpu().numpy().view(np.uint32) != want_ends[src])
    assert bad.size == 0, f"{code.name}: end states differ in {bad.size} of {F} frames, first {bad[0]}"
    bad = np.flatnonzero(ok.cpu().numpy() != want_ok[src])
    assert bad.size == 0, f"{code.name}: flags differ in {bad.size} of {F} frames, first {bad[0]}"


def test_large_batch_soft16_every_frame(oracle):
    """test_side_pass_overhead's batch -- LTE SOFT16, 65536 frames of 40 bits, 4096 distinct repeated -- frame by frame"""
    _large_batch_check(oracle, COMMON_CODES[3], "SOFT16", 65536, 4096, 40, seed=5)


def test_large_batch_int8_every_frame(oracle):
    """DAB K7 R4 HARD8, 8192 frames of 1000 bits from 512 distinct: 2.2 M chunks of 16 int8 symbols"""
    _large_batch_check(oracle, COMMON_CODES[4], "HARD8", 8192, 512, 1000, seed=6)
