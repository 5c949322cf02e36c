"""The single-frame latency route at K = 8 and 9 with R <= 4 (csrc/kernels_one.hpp: one_update_wide_body, one_chainback_body_w,
one_frame_wide_kernel -- lane == state mod 64, two or four states per lane) behind ViterbiDecoder_HIP.update() +
ViterbiDecoder_Core.chainback() of ONE decoder object, and the switch beside it: host_route_note() says which kernel family serves a
code, set_host_route(HOST_ROUTE_LDS) puts the general LDS plan there.  Everything the reference leaves behind is compared with the
oracle -- decision rows (N / 64 words each), metrics, the renormalisation sum, chainback bytes -- and with the LDS route."""
import ctypes as C
import functools
import json
import os
import time

import numpy as np
import pytest

from tests.helpers import decisions_match_fixture, make_table_config, oracle_cfg
from viterbidecodercpp_amd import (COMMON_CODES, Code, ViterbiBranchTable, ViterbiDecoder_Config, ViterbiDecoder_Core, ViterbiDecoder_HIP,
                                   _lib, get_decoding_config, synth)

pytestmark = pytest.mark.gpu

IS95A, CDMA2000 = COMMON_CODES[5], COMMON_CODES[6]
K8R2 = Code("K8 R2", 8, 2, (0o247, 0o371))
K8R3 = Code("K8 R3", 8, 3, (0o225, 0o331, 0o367))
K9R1 = Code("K9 R1", 9, 1, (0o753,))
CODES = [IS95A, CDMA2000, K8R2, K8R3, K9R1]
GROUP = 32                                     # steps the update kernel unrolls: pieces of 31, 32, 33 steps sit around it


def chunk_rows(code):
    """rows the chainback stages per pass: 8192 / (N / 64)"""
    return 8192 // code.decision_words


def shapes(code):
    """(L, pieces): a whole frame; ragged pieces, each its own launch; a frame longer than two chainback chunks; five bits"""
    return ((1300, None), (777, (1, 63, 64, 65, 200, 7, 128, 31, 32, 33)), (2 * chunk_rows(code) + 11, (3000, 1500)), (5, None))


@functools.lru_cache(maxsize=None)
def frames_of(code, decode_type):
    """per shape: symbols, start and end state (both >= 64: registers other than 0 start and end the path) -- made once per (code, type)"""
    pc = get_decoding_config(decode_type, code.R)
    rng = np.random.default_rng(code.K * 100 + code.R)
    out = []
    for L, pieces in shapes(code):
        S = L + code.K - 1
        _, sym = synth.make_frames_numpy(code, pc, 1, (L + 7) // 8 * 8, 2.0, seed=L)     # (the generator wants whole bytes)
        sym = np.ascontiguousarray(sym[:, :S])
        ss, es = int(rng.integers(64, code.num_states)), int(rng.integers(64, code.num_states))
        out.append((L, pieces, sym, ss, es))
    return out


@functools.lru_cache(maxsize=None)
def oracle_results(oracle, code, decode_type):
    cfg = oracle_cfg(decode_type, code.R)
    return [oracle.decode(code.K, code.R, code.G, cfg, sym[0], L, start_state=ss, end_state=es) for L, pieces, sym, ss, es in frames_of(code, decode_type)]


def run_frame(vitdec, code, L, pieces, sym, ss, es, exact):
    """reset -> update (whole, or in pieces) -> everything the decoder leaves behind"""
    S = L + code.K - 1
    flat = sym[0].reshape(-1)
    vitdec.set_traceback_length(L)
    vitdec.set_exact_update_return(exact)        # exact: a piece of 31 steps is a launch of 31 steps, not a queue entry
    vitdec.reset(ss)
    acc, t, k = 0, 0, 0
    while t < S:
        n = S - t if pieces is None else min(pieces[k % len(pieces)], S - t)
        acc += ViterbiDecoder_HIP.update(vitdec, flat[t * code.R:(t + n) * code.R])
        t, k = t + n, k + 1
    acc += vitdec.take_unreported_renormalisation()
    error = vitdec.get_error(es)
    acc += vitdec.take_unreported_renormalisation()
    return dict(error=error, renorm_sum=acc, metrics=vitdec.m_metrics.astype(np.uint32).copy(),
                decisions=np.asarray(vitdec.m_decisions).reshape(S, -1).copy(), bytes=vitdec.chainback(L, es))


def assert_same(got, want, tag):
    assert got["error"] == want["error"], tag
    assert got["renorm_sum"] == want["renorm_sum"], tag
    assert np.array_equal(got["metrics"], want["metrics"]), tag
    S = got["decisions"].shape[0]
    bad = np.argwhere(got["decisions"] != want["decisions"].reshape(S, -1))
    assert bad.size == 0, (tag, "decision words differ first at (row, word)", bad[0], len(bad))
    assert np.array_equal(got["bytes"], want["bytes"]), tag


NOTE_CASES = [(IS95A, "single-frame wide"), (K8R3, "single-frame wide"),
              (Code("K9 R6", 9, 6, (0o753, 0o561, 0o711, 0o663, 0o557, 0o745)), "PLAN_LDS"), (COMMON_CODES[7], "PLAN_LDS"),
              (COMMON_CODES[2], "single-frame in-place (K = 7)")]


def test_route_note_names_the_kernel_family():
    for code, family in NOTE_CASES:
        pc, table, config = make_table_config(code, "SOFT16")
        vitdec = ViterbiDecoder_Core(table, config)
        note = vitdec.host_route_note()
        assert note.startswith(f"K={code.K} R={code.R}: ") and family in note, note
        assert ("PLAN_LDS" in note) == (family == "PLAN_LDS"), note
        if family == "PLAN_LDS":                   # ... and why
            assert ("K >= 10" if code.K >= 10 else "R >= 5") in note, note
        vitdec.set_host_route(_lib.HOST_ROUTE_LDS)
        forced = vitdec.host_route_note()
        assert "PLAN_LDS" in forced and "single-frame" not in forced.split(";")[0], forced
        vitdec.set_host_route(_lib.HOST_ROUTE_AUTO)
        assert vitdec.host_route_note() == note
    lib = _lib.load()
    assert lib.vit_hip_set_host_route(vitdec._handle._h, 7) == _lib.ERR_INVALID_ARG
    assert vitdec.host_route_note() == note


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name.replace(" ", "_"))
def test_wide_single_frame_route_matches_the_oracle(oracle, code, decode_type):
    """whole frame; ragged pieces around the 32-step group and the 64-step deferral limit, every piece a launch of its own; a frame
    longer than two chainback chunks (2048 rows at K = 9, 4096 at K = 8); five bits.  Start and end states >= 64."""
    pc, table, config = make_table_config(code, decode_type)
    vitdec = ViterbiDecoder_Core(table, config)
    assert "single-frame wide" in vitdec.host_route_note()
    for (L, pieces, sym, ss, es), want in zip(frames_of(code, decode_type), oracle_results(oracle, code, decode_type)):
        got = run_frame(vitdec, code, L, pieces, sym, ss, es, exact=pieces is not None and len(pieces) > 2)
        assert got["decisions"].shape == (L + code.K - 1, code.num_states // 64)
        assert_same(got, want, (code.name, decode_type, L, pieces))


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("code", CODES, ids=lambda c: c.name.replace(" ", "_"))
def test_lds_route_gives_what_the_wide_route_gives(oracle, code, decode_type):
    """the same frames under set_host_route(HOST_ROUTE_LDS): rows, metrics, sums and bytes identical to the wide route's and to the
    oracle's; and a frame whose update ran on one route chains back on the other (the device rows stay valid across the switch)"""
    pc, table, config = make_table_config(code, decode_type)
    wide, lds = ViterbiDecoder_Core(table, config), ViterbiDecoder_Core(table, config)
    lds.set_host_route(_lib.HOST_ROUTE_LDS)
    assert "PLAN_LDS" in lds.host_route_note() and "single-frame wide" in wide.host_route_note()
    for (L, pieces, sym, ss, es), want in zip(frames_of(code, decode_type), oracle_results(oracle, code, decode_type)):
        exact = pieces is not None and len(pieces) > 2
        a = run_frame(wide, code, L, pieces, sym, ss, es, exact)
        b = run_frame(lds, code, L, pieces, sym, ss, es, exact)
        assert_same(b, a, (code.name, decode_type, L, pieces, "lds against wide"))
        assert_same(b, want, (code.name, decode_type, L, pieces, "lds against the oracle"))
    # update on the wide route, rows still on the device, chainback of another end state on the LDS route -- and back
    L, pieces, sym, ss, es = frames_of(code, decode_type)[0]
    want = oracle_results(oracle, code, decode_type)[0]
    wide.set_traceback_length(L)
    wide.reset(ss)
    ViterbiDecoder_HIP.update(wide, sym[0].reshape(-1))
    assert wide.rows_on_device == L + code.K - 1
    wide.set_host_route(_lib.HOST_ROUTE_LDS)
    assert np.array_equal(wide.chainback(L, es), want["bytes"])
    wide.set_host_route(_lib.HOST_ROUTE_AUTO)
    assert np.array_equal(wide.chainback(L - 3, 65), oracle.chainback(code.K, want["decisions"], L - 3, 65))
    assert wide.rows_on_device == L + code.K - 1


@pytest.mark.parametrize("width", [2, 1])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [8, 9])
def test_wide_single_frame_kernel_fuzzed(oracle, K, R, width):
    """thresholds of 0 ("always": the late test fires behind every step), of a few steps' error, of the type's maximum; full-range
    garbage symbols (the 16-bit sums wrap); L in 1 .. 700; calls cut into pieces around the 32-step group, each a launch of its own;
    start and end states in every register.  Decision rows, metrics, renormalisation sums, error and bytes against the oracle."""
    from tests.test_gpu_fuzz import random_config

    rng = np.random.default_rng(9000 + 100 * K + 10 * R + width)
    N = 1 << (K - 1)
    G = tuple(int(g) | 1 | N for g in rng.integers(0, 2 * N, R))
    sdt, edt = (np.int16, np.uint16) if width == 2 else (np.int8, np.uint8)
    lim = 1 << (8 * width - 1)
    for trial in range(12):
        cfg = random_config(rng, width, trial % 4)
        if trial >= 8:          # a threshold a few steps' error above the start: state 0 crosses it every two to six steps
            M = (1 << (8 * width)) - 1
            cfg = type(cfg)(width, width, cfg.high, cfg.low, (cfg.high - cfg.low) * R & M, 0, min(M, 3 * ((cfg.high - cfg.low) * R & M)),
                            min(M, 5 * ((cfg.high - cfg.low) * R & M) + 1))
        table = ViterbiBranchTable(K, R, G, cfg.high, cfg.low, sdt)
        config = ViterbiDecoder_Config(cfg.max_error, cfg.initial_start_error, cfg.initial_non_start_error, cfg.renormalisation_threshold, edt)
        L = int(rng.integers(1, 700))
        S = L + K - 1
        if trial % 2:
            sym = rng.integers(cfg.low, cfg.high + 1, size=(S, R)).astype(sdt)
        else:
            sym = rng.integers(-lim, lim, size=(S, R)).astype(sdt)
        ss, es = int(rng.integers(0, N)), int(rng.integers(0, N))
        want = oracle.decode(K, R, G, cfg, sym, L, start_state=ss, end_state=es)
        vitdec = ViterbiDecoder_Core(table, config)
        assert "single-frame wide" in vitdec.host_route_note()
        pieces = None if trial % 3 == 0 else (31, 32, 33, 1, 63, 64, 65, 96, 5)
        got = run_frame(vitdec, Code("fuzz", K, R, G), L, pieces, sym[None], ss, es, exact=trial % 3 == 1)
        assert_same(got, want, (K, R, width, trial, L, cfg))


@pytest.mark.parametrize("K", [8, 9])
def test_wide_parallel_chainback_is_exact_when_its_guesses_are_wrong(oracle, K):
    """rows of random bits keep survivor paths apart: every guessed top state is wrong and the repair pass does the work; rows of
    zeros and rows that repeat with a short period stress the boundaries.  Lengths: whole chunks, a ragged top byte, three chunks, frames
    shorter than 64 segments."""
    code = Code(f"K{K}", K, 2, ((1 << K) - 1, (1 << (K - 1)) | 1))
    pc, table, config = make_table_config(code, "SOFT16")
    vitdec = ViterbiDecoder_Core(table, config)           # only its handle is used: the rows below are not a decoder's
    lib = _lib.load()
    rng = np.random.default_rng(K)
    N, W, chunk = code.num_states, code.decision_words, chunk_rows(code)
    for L in (chunk, chunk - 1, 2 * chunk + 301, 2 * chunk + 8, 517, 64, 9, 1):
        S = L + K - 1
        for kind in ("random", "zeros", "period3"):
            if kind == "random":
                rows = rng.integers(0, 1 << 63, size=(S, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(S, W)).astype(np.uint64)
            elif kind == "zeros":
                rows = np.zeros((S, W), dtype=np.uint64)
            else:
                rows = np.ascontiguousarray(np.tile(rng.integers(0, 1 << 62, size=(3, W), dtype=np.uint64), (S // 3 + 1, 1))[:S])
            for es in (0, N - 1, int(rng.integers(64, N))):
                want = oracle.chainback(K, rows, L, es)
                out = np.zeros((L + 7) // 8, dtype=np.uint8)
                assert lib.vit_hip_chainback_host(vitdec._handle._h, rows.ctypes.data_as(C.c_void_p), L, es, out.ctypes.data_as(C.c_void_p)) == _lib.OK
                assert np.array_equal(out, want), (L, kind, es)


@pytest.mark.parametrize("code,decode_type", [(IS95A, "SOFT16"), (CDMA2000, "SOFT8")], ids=lambda x: x.name.replace(" ", "_") if hasattr(x, "name") else x)
def test_wide_frame_route_keeps_rows_on_the_device(oracle, code, decode_type):
    """the one-launch frame: update() leaves its rows in the device row store and chains the completed frame back; reading m_decisions
    brings them home, bit for bit the reference's; rows CHANGED on the host are what the next chainback follows"""
    pc, table, config = make_table_config(code, decode_type)
    cfg = oracle_cfg(decode_type, code.R)
    L = 1544
    S, N = L + code.K - 1, code.num_states
    vitdec = ViterbiDecoder_Core(table, config)
    assert "single-frame wide" in vitdec.host_route_note()
    vitdec.set_traceback_length(L)
    for frame, pieces in enumerate((None, (700, 65, 200), None)):
        _, sym = synth.make_frames_numpy(code, pc, 1, L, 2.0, seed=80 + frame)
        flat = sym[0].reshape(-1)
        want0 = oracle.decode(code.K, code.R, code.G, cfg, sym[0], L)
        vitdec.reset()
        acc, t, k = 0, 0, 0
        while t < S:
            n = S - t if pieces is None else min(pieces[k % len(pieces)], S - t)
            acc += ViterbiDecoder_HIP.update(vitdec, flat[t * code.R:(t + n) * code.R])
            t, k = t + n, k + 1
        assert acc == want0["renorm_sum"] and vitdec.rows_on_device == S
        assert np.array_equal(vitdec.chainback(L), want0["bytes"])                       # decoded by the completing update
        assert vitdec.rows_on_device == S                                                # nothing came home for that
        es = N - 1
        assert np.array_equal(vitdec.chainback(L, es), oracle.chainback(code.K, want0["decisions"], L, es))          # another end state: one kernel
        assert np.array_equal(vitdec.chainback(L - 11, 131), oracle.chainback(code.K, want0["decisions"], L - 11, 131))   # fewer bits, ragged
        assert vitdec.get_error(0) == want0["error"] and vitdec.rows_on_device == S
    rows = vitdec.m_decisions                                                            # rows come home; the array is the caller's to change
    assert vitdec.rows_on_device == 0 and rows.shape == (S, N // 64)
    assert np.array_equal(np.asarray(rows), want0["decisions"].reshape(S, -1))
    rng = np.random.default_rng(7)
    rows[100:900] ^= rng.integers(0, 1 << 63, size=rows[100:900].shape, dtype=np.uint64)
    assert not np.array_equal(oracle.chainback(code.K, np.asarray(rows), L, 1), oracle.chainback(code.K, want0["decisions"], L, 1))
    assert np.array_equal(vitdec.chainback(L, 1), oracle.chainback(code.K, np.asarray(rows), L, 1))
    # and the decoder goes on: the next frame is lazy again
    vitdec.reset()
    ViterbiDecoder_HIP.update(vitdec, flat)
    assert vitdec.rows_on_device == S and np.array_equal(vitdec.chainback(L), want0["bytes"])


@pytest.mark.parametrize("name", ["k9r2_soft16_2db", "k9r2_soft16_2db_l4096"])
def test_wide_route_decodes_the_golden_frames(name):
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    meta = json.load(open(os.path.join(gold, "MANIFEST.json")))[name]
    g = np.load(os.path.join(gold, name + ".npz"))
    pc = get_decoding_config(meta["decode_type"], meta["R"])
    table = ViterbiBranchTable(meta["K"], meta["R"], meta["G"], pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    vitdec = ViterbiDecoder_Core(table, ViterbiDecoder_Config.from_decoder_config(pc))
    assert "single-frame wide" in vitdec.host_route_note()
    L = meta["L"]
    vitdec.set_traceback_length(L)
    vitdec.reset(meta["start_state"])
    acc = ViterbiDecoder_HIP.update(vitdec, g["symbols"].reshape(-1))
    assert vitdec.m_current_decoded_bit == meta["steps"]
    assert acc == int(g["renorm_sum"])
    assert np.array_equal(vitdec.chainback(L, meta["end_state"]), g["bytes"])            # (first: off the device rows)
    assert vitdec.get_error(meta["end_state"]) == int(g["error"])
    assert np.array_equal(vitdec.m_metrics.astype(np.uint32), g["metrics"])
    assert decisions_match_fixture(vitdec.m_decisions, g)
    assert np.array_equal(vitdec.chainback(L, meta["end_state"]), g["bytes"])            # (again: off the host rows)


def test_wide_route_is_worth_its_code(oracle):
    """one 4096-bit IS-95A SOFT16 frame, reset -> update -> chainback on one decoder object, 8 repetitions under each route in one
    process: the median of the last 6 under AUTO must be at most 0.75 of that under HOST_ROUTE_LDS.  The 0.75 is the condition that
    the route is worth its code, not a measurement; both sides are timed in the same run on the same box."""
    code = IS95A
    pc, table, config = make_table_config(code, "SOFT16")
    L = 4096
    _, sym = synth.make_frames_numpy(code, pc, 1, L, 3.0, seed=3)
    flat = sym[0].reshape(-1)
    want = oracle.decode(code.K, code.R, code.G, oracle_cfg("SOFT16", code.R), sym[0], L)["bytes"]
    vitdec = ViterbiDecoder_Core(table, config)
    vitdec.set_traceback_length(L)
    medians = {}
    for route in (_lib.HOST_ROUTE_AUTO, _lib.HOST_ROUTE_LDS):
        vitdec.set_host_route(route)
        times = []
        for rep in range(8):
            vitdec.reset()
            t0 = time.perf_counter()
            ViterbiDecoder_HIP.update(vitdec, flat)
            out = vitdec.chainback(L)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(out, want)
        medians[route] = float(np.median(times[2:]))
    t_auto, t_lds = medians[_lib.HOST_ROUTE_AUTO], medians[_lib.HOST_ROUTE_LDS]
    print(f"single 4096-bit IS-95A SOFT16 frame, update + chainback through the drop-in: wide {t_auto * 1e3:.3f} ms, "
          f"PLAN_LDS on one frame {t_lds * 1e3:.3f} ms, ratio {t_auto / t_lds:.3f}")
    assert t_auto <= 0.75 * t_lds, (t_auto, t_lds)
