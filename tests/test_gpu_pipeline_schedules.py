"""vit_hip_pipeline_create_ex: every schedule override, batches that are split into sub-batches, and per-frame end states.

The rest of the suite runs the pipeline in one shape: the schedule the rules pick, whole batches, d_end_state = NULL.  Here every
override branch of pipeline_schedule() (csrc/vit_pipeline.hip) runs under one pipeline each -- three update streams, two to four
workspaces, fewer workspaces than update streams, the small chainback kernel inside a two-update schedule, forced overlap on
PLAN_LDS / PLAN_LDS2 -- with batches of 2 x per_wave + per_wave / 8 + 1 frames that the sub-batch loop of submit() cuts into three
(the last one ragged: a partial tile, a partial frame pair), and with per-frame end states on every other submission.

References, all bit exact: the serial route on the same decoder (update, then chainback with the same end states) over every
frame; the CPU oracle on the frames around every sub-batch boundary, bytes and decision rows.

per_wave = 4 x CUs x tile frames is one update wave per SIMD (reg_plan.hpp: tile = 32 frames from K = 7 on, 128 below): every
expectation is computed from the device's CU count.  No torch stream is created here: torch's default current stream is enough,
and extra streams would shift torch's stream pool under tests/test_gpu_residency.py."""
import ctypes as C

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, Code, DecodePipeline, _lib
from tests.helpers import make_table_config, oracle_cfg

pytestmark = pytest.mark.gpu

Opt = _lib.VitHipPipelineOptions

VOYAGER16 = (2, "SOFT16")
VOYAGER_HARD = (2, "HARD8")
IS95 = (5, "SOFT16")
LTE = (3, "SOFT16")
K5 = (1, "SOFT8")
K11 = ((11, 2, (0o3345, 0o3613)), "SOFT16")        # PLAN_LDS2
K6R3 = ((6, 3, (0o65, 0o57, 0o75)), "SOFT16")       # PLAN_LDS
REG_CODES = [VOYAGER16, VOYAGER_HARD, IS95, LTE, K5]
LDS_CODES = [K11, K6R3]
EBN0 = {"SOFT16": 2.0, "SOFT8": 3.0, "HARD8": 4.0}


def _code(key):
    return COMMON_CODES[key[0]] if isinstance(key[0], int) else Code(f"K{key[0][0]}R{key[0][1]}", *key[0])


def _key_id(key):
    c = _code(key)
    return f"K{c.K}R{c.R}-{key[1]}"


_decoders = {}


def _decoder(key):
    """one decoder per code for the whole file: (code, decoder, L)"""
    if key not in _decoders:
        code = _code(key)
        pc, table, config = make_table_config(code, key[1])
        dec = BatchDecoder(table, config)
        L = 64 if dec.plan != _lib.PLAN_REG else (40 if code.K >= 7 else 24)
        _decoders[key] = (code, dec, L)
    return _decoders[key]


def _per_wave(key):
    """frames of one update wave per SIMD, from the device's CU count; 0 off the register plan"""
    import torch

    code, dec, _ = _decoder(key)
    if dec.plan != _lib.PLAN_REG:
        return 0
    return 4 * torch.cuda.get_device_properties(dec.device).multi_processor_count * (32 if code.K >= 7 else 128)


def _split_frames(key):
    """three sub-batches of per_wave, the last one ragged: it ends in a partial tile and a partial frame pair"""
    pw = _per_wave(key)
    return 2 * pw + pw // 8 + 1


_batches = {}


def _batch(key, n, seed, with_end_state):
    """(symbols, transmitted bytes, end states or None, bytes of the serial route) of one submission; made once per
    (code, frames, seed) and only read afterwards"""
    import torch

    k = (key, n, seed, with_end_state)
    if k not in _batches:
        code, dec, L = _decoder(key)
        tx, sym = dec.synth(n, L, EBN0[key[1]], seed=seed)
        es = None
        if with_end_state:
            es = torch.from_numpy(np.random.default_rng(seed).integers(0, code.num_states, n).astype(np.int32)).to(dec.device)
        dec.update(sym, L, want_metrics=False)
        ref = dec.chainback(n, L, end_state=es)
        torch.cuda.synchronize()
        _batches[k] = (sym, tx, es, ref)
    return _batches[k]


def _schedule(pipe):
    s = pipe.schedule
    return dict(workspaces=s.workspaces, update_streams=s.update_streams, overlapped=s.chainback_overlapped,
                priority=s.chainback_wave_priority, sub=int(s.sub_batch_frames), small=s.chainback_small_kernel)


def _counts(max_frames, sub, n_submissions):
    cycle = (max_frames, max_frames, sub, sub + 1, 1, max_frames, max(max_frames // 3, 1))
    return [min(cycle[i % len(cycle)], max_frames) for i in range(n_submissions)]


def _sample_frames(n, sub):
    return sorted({f for f in (0, sub - 1, sub, 2 * sub - 1, 2 * sub, n - 1) if 0 <= f < n})


def _oracle_frame(oracle, key, sym, f, es):
    code, _, L = _decoder(key)
    return oracle.decode(code.K, code.R, code.G, oracle_cfg(key[1], code.R), sym[f].cpu().numpy(), L,
                         end_state=0 if es is None else int(es[f].item()))


def _run_row(oracle, key, max_frames, opt, want, seed0):
    """one pipeline with the options of a row: its reported schedule, then 2 x workspaces + 1 submissions against both references"""
    import torch

    code, dec, L = _decoder(key)
    lib = _lib.load()
    pipe = DecodePipeline(dec, max_frames, L, options=opt)
    try:
        sch = _schedule(pipe)
        tag = f"{_key_id(key)} max_frames={max_frames} schedule={sch}"
        for field, value in want.items():
            assert sch[field] == value, f"{field}: {tag}"
        sub = sch["sub"]
        assert pipe.schedule.workspace_bytes_each == dec.workspace_bytes(min(max_frames, sub), L), tag
        pipe.set_timing(True)
        counts = _counts(max_frames, sub, max(7, 2 * sch["workspaces"] + 1))
        subs = []
        for i, n in enumerate(counts):
            sym, tx, es, ref = _batch(key, n, seed0 + i, i % 2 == 1)
            out = torch.full((n + 2, (L + 7) // 8), 0xA5, dtype=torch.uint8, device=dec.device)
            subs.append((n, sym, es, ref, out))
        for n, sym, es, ref, out in subs:                        # no host synchronisation between the submissions
            pipe.submit(sym, out[:n], end_state=es)
        sym0, out0 = subs[0][1], subs[0][4]
        ptr = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
        assert lib.vit_hip_pipeline_submit(pipe._p, ptr(sym0), max_frames + 1, ptr(out0), None, None) == _lib.ERR_INVALID_ARG, tag
        assert lib.vit_hip_pipeline_submit(pipe._p, ptr(sym0), 0, ptr(out0), None, None) == _lib.OK, tag
        pipe.sync()
        for i, (n, sym, es, ref, out) in enumerate(subs):
            bad = (out[:n] != ref).any(dim=1).nonzero().flatten()
            assert torch.equal(out[:n], ref), f"submission {i} of {n} frames: {bad.numel()} frames differ from the serial route, first {bad[:4].tolist()}: {tag}"
            assert bool((out[n:] == 0xA5).all()), f"submission {i}: guard rows behind frame {n} were written: {tag}"
        # the oracle around every sub-batch boundary: one submission without end states, one with
        for i in (0, 1):
            n, sym, es, ref, out = subs[i]
            assert (es is None) == (i == 0)
            for f in _sample_frames(n, sub):
                want_bytes = _oracle_frame(oracle, key, sym, f, es)["bytes"]
                assert np.array_equal(out[f].cpu().numpy(), want_bytes), f"submission {i} frame {f} differs from the oracle: {tag}"
        # the decision rows of the last sub-batch of the last submission
        n, sym, es, ref, out = subs[-1]
        f0, rows = pipe.export_last_decisions()
        nf = rows.shape[0]
        assert (f0, nf) == ((n - 1) // sub * sub, n - (n - 1) // sub * sub), tag
        dec.update(sym[f0:f0 + nf].contiguous(), L, want_metrics=False)
        assert torch.equal(rows, dec.export_decisions(nf, L)), f"decision rows of frames {f0}..{f0 + nf - 1}: {tag}"
        want_rows = _oracle_frame(oracle, key, sym, f0, es)["decisions"]
        assert np.array_equal(rows[0].cpu().numpy().view(np.uint64), want_rows), f"decision rows of frame {f0} differ from the oracle: {tag}"
        # one timing record per sub-batch, in submit order
        u, c, d = pipe.timing()
        assert len(u) == len(c) == len(d) == sum(-(-n // sub) for n in counts), tag
        assert (u > 0).all() and (c > 0).all() and (d > 0).all(), tag
        if sch["update_streams"] > 1:                            # all chainbacks share one stream there
            assert (np.diff(d) >= 0).all(), tag
    finally:
        pipe.close()
    return sch


def _rows():
    """(row, code, max_frames as a function of the code, options, reported schedule as a function of the code)"""
    pw, F = _per_wave, _split_frames
    k7 = lambda key: _code(key).K == 7                           # noqa: E731
    rows = []
    for key in REG_CODES:
        rows += [
            ("A", key, F, dict(sub_batches=1),
             lambda k: dict(sub=pw(k), update_streams=2, workspaces=3, overlapped=1, priority=1, small=0)),
            ("B", key, F, dict(sub_batches=1, update_streams=3),
             lambda k: dict(sub=pw(k), update_streams=3, workspaces=4, overlapped=1, priority=1, small=0)),
            # fewer workspaces than update streams: only the wait on the workspace's last chainback keeps its reuse correct
            ("C", key, F, dict(sub_batches=1, update_streams=3, workspaces=2),
             lambda k: dict(sub=pw(k), update_streams=3, workspaces=2, overlapped=1, priority=1, small=0)),
            # sub-batches are fed from two update streams: the request for one is the field that is ignored
            ("D", key, F, dict(sub_batches=1, update_streams=1),
             lambda k: dict(sub=pw(k), update_streams=2, workspaces=3, overlapped=1, priority=1, small=0)),
            ("E", key, F, dict(sub_batches=1, chainback_small_kernel=1, chainback_wave_priority=0),
             lambda k: dict(sub=pw(k), update_streams=2, workspaces=3, overlapped=1, priority=0, small=1 if k7(k) else 0)),
            ("F", key, pw, dict(chainback_overlap=0, sub_batches=0, update_streams=1),
             lambda k: dict(sub=pw(k), update_streams=1, workspaces=2, overlapped=0, priority=0, small=0)),
        ]
    for key in (VOYAGER16, VOYAGER_HARD):
        rows += [
            ("G", key, lambda k: 4 * pw(k) + 1, dict(chainback_overlap=1),
             lambda k: dict(sub=4 * pw(k) + 1, update_streams=1, workspaces=2, overlapped=1, priority=0, small=1)),
            # the LDS-ring chainback inside the two-update schedule
            ("I", key, lambda k: 2048, dict(update_streams=2, chainback_small_kernel=1, chainback_wave_priority=1),
             lambda k: dict(sub=2048, update_streams=2, workspaces=3, overlapped=1, priority=1, small=1)),
        ]
    for key in (VOYAGER16, VOYAGER_HARD, IS95):
        rows.append(("H", key, lambda k: 2048, dict(update_streams=2, workspaces=4),
                     lambda k: dict(sub=2048, update_streams=2, workspaces=4, overlapped=1, priority=1, small=0)))
    for key in LDS_CODES:
        # K = 6, R = 3 (PLAN_LDS): the rules never overlap; K = 11 (PLAN_LDS2): they do.  Forced, both take two update streams.
        rows.append(("J", key, lambda k: 200, dict(chainback_overlap=1, update_streams=2),
                     lambda k: dict(sub=200, update_streams=2, workspaces=3, overlapped=1, priority=1, small=0)))
    # no sub-batches and no third update stream off the register plan; two update streams wherever the chainback is overlapped
    rows.append(("K", K11, lambda k: 200, dict(sub_batches=1, update_streams=3),
                 lambda k: dict(sub=200, update_streams=2, workspaces=3, overlapped=1, priority=1, small=0)))
    rows.append(("K", K6R3, lambda k: 200, dict(sub_batches=1, update_streams=3),
                 lambda k: dict(sub=200, update_streams=1, workspaces=2, overlapped=0, priority=0, small=0)))
    return rows


ROWS = _rows()
RULES_PICK = {"F": (3, 2, 1), "G": (2, 1, 0)}      # (workspaces, update streams, overlapped) of vit_hip_pipeline_create at that max_frames


@pytest.mark.parametrize("key", REG_CODES, ids=_key_id)
def test_per_wave_is_the_two_update_limit_the_rules_report(key):
    """4 x CUs x tile, computed here from the CU count, is what a rule-made pipeline reports as the largest two-update batch"""
    code, dec, L = _decoder(key)
    assert dec.plan == _lib.PLAN_REG
    dec._handle.refresh()
    assert dec._handle.info.workspace_tile_frames == (32 if code.K >= 7 else 128)
    pipe = DecodePipeline(dec, 1, L)
    try:
        assert int(pipe.schedule.two_updates_max_frames) == _per_wave(key) > 0
        assert (pipe.schedule.workspaces, pipe.schedule.update_streams, int(pipe.schedule.sub_batch_frames)) == (3, 2, 1)
    finally:
        pipe.close()


@pytest.mark.parametrize("row,key,max_frames,opt,want", ROWS, ids=[f"{r[0]}-{_key_id(r[1])}" for r in ROWS])
def test_schedule_override_matches_serial_route_and_oracle(oracle, row, key, max_frames, opt, want):
    """one option row: the schedule vit_hip_pipeline_get_schedule_v2 reports, then 2 x workspaces + 1 submissions (every workspace
    reused at least twice; whole batches, exactly one sub-batch, one frame more, one frame, a third) with their own symbols,
    end states on every other one and two guard rows behind every output"""
    code, dec, L = _decoder(key)
    assert dec.plan == {K11: _lib.PLAN_LDS2, K6R3: _lib.PLAN_LDS}.get(key, _lib.PLAN_REG)
    F = max_frames(key)
    if row in RULES_PICK:
        pipe = DecodePipeline(dec, F, L)
        try:
            s = pipe.schedule
            assert (s.workspaces, s.update_streams, s.chainback_overlapped) == RULES_PICK[row] and int(s.sub_batch_frames) == F
        finally:
            pipe.close()
    sch = _run_row(oracle, key, F, Opt(**opt), want(key), seed0=1000)
    if row in "ABCDE":
        assert sch["sub"] < F <= 3 * sch["sub"] and F % 32 and F % 2       # three sub-batches, the last one ragged


@pytest.mark.parametrize("opt", [dict(sub_batches=1), dict(sub_batches=1, update_streams=3)], ids=["A", "B"])
def test_done_event_covers_every_sub_batch(opt):
    """submit -> wait_done -> a consumer on torch's current stream, no host synchronisation: done_event is recorded behind the
    LAST sub-batch's chainback and all chainbacks share one stream, so the consumer sees the bytes of all three sub-batches"""
    import torch

    key = VOYAGER16
    code, dec, L = _decoder(key)
    F = _split_frames(key)
    pipe = DecodePipeline(dec, F, L, options=Opt(**opt))
    try:
        assert int(pipe.schedule.sub_batch_frames) == _per_wave(key)
        runs = []
        batches = [_batch(key, F, 1000 + i, i % 2 == 1) for i in range(4)]
        for sym, tx, es, ref in batches:
            out = torch.full((F, (L + 7) // 8), 0xA5, dtype=torch.uint8, device=dec.device)
            pipe.submit(sym, out, end_state=es)
            pipe.wait_done()
            runs.append((out, tx, ref, torch.bitwise_xor(out, tx).sum(dim=1)))     # per frame: which sub-batch was late is visible
        torch.cuda.synchronize()
        for i, (out, tx, ref, x) in enumerate(runs):
            assert torch.equal(out, ref), f"submission {i}"
            late = (x != torch.bitwise_xor(ref, tx).sum(dim=1)).nonzero().flatten()
            assert late.numel() == 0, f"submission {i}: the consumer read {late.numel()} unfinished frames, first {late[:4].tolist()}"
    finally:
        pipe.close()


def _raw_options(struct_size, fields, trailing=()):
    """a vit_hip_pipeline_options image of int32 words: struct_size, the six fields, then `trailing` words behind the struct"""
    words = (C.c_int32 * (7 + len(trailing)))(struct_size, *fields, *trailing)
    return words


def test_options_struct_size_and_ranges():
    """the struct_size prefix copy (shorter: only the prefix is read; longer: the tail is ignored) and every range check"""
    code, dec, L = _decoder(VOYAGER16)
    lib = _lib.load()
    F = 64
    pw = _per_wave(VOYAGER16)

    def create(words):
        pipe = C.c_void_p(0xDEAD)
        rc = lib.vit_hip_pipeline_create_ex(dec._handle._h, F, L, C.cast(words, C.POINTER(Opt)), C.byref(pipe))
        sch = None
        if rc == _lib.OK:
            sch = _lib.VitHipPipelineSchedule()
            assert lib.vit_hip_pipeline_get_schedule_v2(pipe, C.byref(sch), C.sizeof(sch)) == _lib.OK
            assert lib.vit_hip_pipeline_destroy(pipe) == _lib.OK
        else:
            assert pipe.value is None, "a failed create leaves *out NULL"
        return rc, sch

    size = C.sizeof(Opt)
    assert size == 28
    rule = (-1, 0, -1, 0, -1, -1)
    rc, base = create(_raw_options(size, rule))
    assert rc == _lib.OK and (base.workspaces, base.update_streams, base.chainback_overlapped) == (3, 2, 1)
    assert base.overlap_max_frames == 3 * pw and base.two_updates_max_frames == pw
    # too short to hold one field
    assert create(_raw_options(4, rule))[0] == _lib.ERR_INVALID_ARG
    assert create(_raw_options(0, rule))[0] == _lib.ERR_INVALID_ARG
    # the 8-byte prefix: chainback_overlap = 0 is read, the out-of-range words behind it are not
    rc, sch = create(_raw_options(8, (0, 99, -7, 1, 5, 0x7FFFFFFF)))
    assert rc == _lib.OK and sch.overlap_max_frames == 0
    assert (sch.workspaces, sch.update_streams, sch.two_updates_max_frames) == (3, 2, pw)      # the other fields: the rules
    # ... and the same words in a struct that says it holds them are refused
    assert create(_raw_options(size, (0, 99, -7, 1, 5, 0x7FFFFFFF)))[0] == _lib.ERR_INVALID_ARG
    # a caller built against a LONGER struct: the words this library does not know are ignored
    rc, sch = create(_raw_options(size + 16, (0, 1, -1, 0, -1, -1), trailing=(0x7FFFFFFF, -99, 5, -1)))
    assert rc == _lib.OK and (sch.workspaces, sch.update_streams, sch.chainback_overlapped) == (2, 1, 0)
    # every field one past either end of its range
    ranges = [(-1, 1), (0, 3), (-1, 1), (2, 4), (-1, 1), (-1, 1)]
    for i, (lo, hi) in enumerate(ranges):
        for v in (lo - 1, hi + 1) + ((-1,) if i == 3 else ()):       # workspaces: 0 (rule) or 2 .. 4, so 1, 5 and -1
            f = list(rule)
            f[i] = v
            assert create(_raw_options(size, f))[0] == _lib.ERR_INVALID_ARG, (Opt._fields_[i + 1][0], v)
        for v in (lo, hi):
            f = list(rule)
            f[i] = v
            assert create(_raw_options(size, f))[0] == _lib.OK, (Opt._fields_[i + 1][0], v)


def test_schedule_struct_truncation():
    """_v2 writes at most schedule_bytes; the legacy entry point writes the struct up to and including `reserved`"""
    code, dec, L = _decoder(VOYAGER16)
    lib = _lib.load()
    pipe = DecodePipeline(dec, 64, L, options=Opt(chainback_small_kernel=1))
    try:
        Sch = _lib.VitHipPipelineSchedule
        size = C.sizeof(Sch)
        assert size == 56 and Sch.reserved.offset + 4 == size
        full = bytes(pipe.schedule)
        assert pipe.schedule.chainback_small_kernel == 1 and pipe.schedule.reserved == 0
        sentinel = lambda: (C.c_ubyte * (size + 16))(*([0xFF] * (size + 16)))     # noqa: E731
        for n in (0, 12, 20, size, size + 16):
            buf = sentinel()
            assert lib.vit_hip_pipeline_get_schedule_v2(pipe._p, C.cast(buf, C.POINTER(Sch)), n) == _lib.OK
            k = min(n, size)
            assert bytes(buf[:k]) == full[:k] and bytes(buf[k:]) == b"\xff" * (size + 16 - k), n
        buf = sentinel()
        assert lib.vit_hip_pipeline_get_schedule(pipe._p, C.cast(buf, C.POINTER(Sch))) == _lib.OK
        assert bytes(buf[:size]) == full and bytes(buf[size:]) == b"\xff" * 16
    finally:
        pipe.close()


def _walk_options(i):
    """the i-th of 12 seeded valid option structs and its max_frames"""
    rng = np.random.default_rng(20240 + i)
    opt = dict(chainback_overlap=int(rng.integers(-1, 2)), update_streams=int(rng.integers(0, 4)), sub_batches=int(rng.integers(-1, 2)),
               workspaces=int(rng.choice([0, 2, 3, 4])), chainback_small_kernel=int(rng.integers(-1, 2)),
               chainback_wave_priority=int(rng.integers(-1, 2)))
    return opt, int(rng.integers(0, 4))


@pytest.mark.parametrize("i", range(12))
def test_seeded_walk_over_valid_options(i):
    """random valid options at the four batch sizes where the rules change: four submissions, end states on two, against the
    serial route"""
    import torch

    key = VOYAGER16
    code, dec, L = _decoder(key)
    opt, which = _walk_options(i)
    pw = _per_wave(key)
    max_frames = (2048, pw, pw + 1, _split_frames(key))[which]
    pipe = DecodePipeline(dec, max_frames, L, options=Opt(**opt))
    try:
        sch = _schedule(pipe)
        tag = f"options={tuple(opt.items())} max_frames={max_frames} schedule={sch}"
        sub = sch["sub"]
        assert 2 <= sch["workspaces"] <= 4 and 1 <= sch["update_streams"] <= 3 and 0 < sub <= max_frames, tag
        if opt["workspaces"]:
            assert sch["workspaces"] == opt["workspaces"], tag
        counts = [max_frames, min(sub + 1, max_frames), max(max_frames // 3, 1), max_frames]
        subs = []
        batches = [_batch(key, n, 1000 + j, j % 2 == 1) for j, n in enumerate(counts)]
        for n, (sym, tx, es, ref) in zip(counts, batches):
            out = torch.full((n + 2, (L + 7) // 8), 0xA5, dtype=torch.uint8, device=dec.device)
            pipe.submit(sym, out[:n], end_state=es)
            subs.append((n, ref, out))
        pipe.sync()
        for j, (n, ref, out) in enumerate(subs):
            assert torch.equal(out[:n], ref), f"submission {j} of {n} frames: {tag}"
            assert bool((out[n:] == 0xA5).all()), f"submission {j}: guard rows: {tag}"
    finally:
        pipe.close()
