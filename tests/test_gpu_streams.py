"""Many lockstep streams decoded in one call on one shared window grid (vit_hip_decode_streams) against the single-stream rule
restated on the CPU checker (tests/stream_reference.py) per stream, and against vit_hip_decode_stream per stream on the same data:
bit for bit on every plan, poisoned padding and output rows, argument errors, graph capture, concurrency, MultiStreamDecoder, and
the time against what one stream per call costs."""
import ctypes as C
import time

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, Code, MultiStreamDecoder, _lib
from tests.helpers import DECODE_TYPES, make_table_config, oracle_cfg
from tests.stream_reference import BEGIN, END, default_extension, make_stream, stream_reference
from tests.streams_reference import streams_windows

pytestmark = pytest.mark.gpu


def _no_compiler(monkeypatch, tmp_path):
    """as tests/test_gpu_generic.py: no hipcc and an empty user cache, so a code outside the stock table runs the GENERIC kernels"""
    monkeypatch.setenv("VIT_HIP_HIPCC", "/nonexistent/hipcc")
    monkeypatch.setenv("VIT_HIP_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("VIT_HIP_JIT", raising=False)


def grid_cases(K, tile):
    """(n_streams, T, W, head, tail, flags, extra pitch in windows).  n_streams 1, 2, 3 and tile + 1 (the remainder batch, and under
    END the kept end states, go beyond one tile; with 2 windows per stream every tile of grid windows straddles many streams);
    1, 2, tile - 1 and tile + 1 windows per stream; all four flag values; W off the byte grid; the smallest pitch and a larger
    one; uniform segments, segments with a longer last window, streams that are one window of their own length (no grid at all),
    the minima of W / head / tail, and head + tail > W (two bridge windows at the smallest pitch)."""
    d = default_extension(K)
    m = K - 1
    Wmin = max(8, m)
    Wd = max(64, d)
    Wo = Wd + 3                                                          # not a multiple of 8
    lo, hi = max(tile - 1, 1), tile + 1
    return [
        (1, d + Wd + d, Wd, d, d, BEGIN, 0),                             # one stream, one window
        (1, d + 2 * Wo + d + 21, Wo, d, d, BEGIN | END, 2),
        (2, d + 2 * Wo + d, Wo, d, d, 0, 0),
        (2, d + lo * Wd + d + 29, Wd, d, d, 0, 1),                       # a longer last window without END: its own select
        (2, d + d + 9, Wd, d, d, BEGIN | END, 0),                        # n = 1, shorter than a window: nothing on the grid
        (3, d + lo * Wo + d, Wo, d, d, BEGIN, 1),
        (3, d + hi * Wd + d + 37, Wd, d, d, BEGIN | END, 0),
        (3, d + Wd + d, Wd, d, d, END, 0),                               # one uniform window per stream, every one ends in state 0
        (3, (m + 2) + 5 * (Wmin + 5) + (m + 4) + 3, Wmin + 5, m + 2, m + 4, END, 0),     # odd W / head / tail
        (3, m + hi * Wmin + m, Wmin, m, m, BEGIN, 0),                    # the minima
        (2, (Wd - 1) + 3 * Wd + (Wd - 1), Wd, Wd - 1, Wd - 1, BEGIN | END, 0),           # head + tail > W
        (tile + 1, d + 2 * Wo + d, Wo, d, d, END, 0),                    # uniform under END: kept end states in every tile
        (tile + 1, d + 2 * Wd + d, Wd, d, d, BEGIN, 3),
        (tile + 1, d + Wd + d + 11, Wd, d, d, 0, 2),                     # one longer window per stream: the remainder batch alone
        (tile + 1, d + 2 * Wd + d + 11, Wd, d, d, BEGIN | END, 0),
    ]


def decode_and_compare(oracle, code, decode_type, dec, streams, pitch, W, head, tail, flags, extra_out, poison=0xA5):
    """one call through the C ABI on a buffer of exactly (n_streams - 1) pitch + T steps with random symbols in the padding and a
    poisoned output, against the restatement per stream and against vit_hip_decode_stream per stream"""
    import torch

    lib, h = _lib.load(), dec._handle._h
    ns, T = len(streams), streams[0].shape[0]
    rng = np.random.default_rng(ns * 1000 + T)
    buf = np.empty(((ns - 1) * pitch + T, code.R), dtype=streams[0].dtype)
    info = np.iinfo(buf.dtype)
    buf[:] = rng.integers(0, 2, size=buf.shape) if decode_type == "HARD8" else rng.integers(info.min // 2, info.max // 2, size=buf.shape)
    for s, sym in enumerate(streams):
        buf[s * pitch:s * pitch + T] = sym
    d_buf = torch.from_numpy(buf).cuda()
    need = lib.vit_hip_streams_workspace_bytes(h, ns, pitch, T, W, head, tail, flags)
    tag = (code.name, decode_type, ns, pitch, T, W, head, tail, flags, _lib.PLAN_NAMES[dec.plan])
    assert need > 0 and need % 256 == 0, tag
    assert need == dec.streams_workspace_bytes(ns, pitch, T, bool(flags & BEGIN), bool(flags & END), W, head, tail)
    ws = torch.full((need,), poison, dtype=torch.uint8, device="cuda")
    want = [stream_reference(oracle, code, oracle_cfg(decode_type, code.R), sym, W, head, tail, flags) for sym in streams]
    nb, want_n = want[0][0].size, want[0][1]
    out_pitch = nb + extra_out
    off = 16 if extra_out % 16 == 0 else 3                           # aligned rows take the 16-byte stores, the others do not
    out = torch.full((off + ns * out_pitch + 32,), poison, dtype=torch.uint8, device="cuda")
    n_bits = C.c_size_t(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.vit_hip_decode_streams(h, C.c_void_p(d_buf.data_ptr()), ns, pitch, T, W, head, tail, flags, C.c_void_p(ws.data_ptr()), need,
                                    C.c_void_p(out.data_ptr() + off), out_pitch, C.byref(n_bits), stream)
    assert rc == _lib.OK, (tag, lib.vit_hip_last_error())
    torch.cuda.synchronize()
    assert n_bits.value == want_n, tag
    host = out.cpu().numpy()
    assert np.all(host[:off] == poison), f"{tag}: wrote in front of the output"
    rows = host[off:off + ns * out_pitch].reshape(ns, out_pitch)
    assert np.all(host[off + ns * out_pitch:] == poison), f"{tag}: wrote behind the output"
    for s in range(ns):
        bad = np.argwhere(rows[s, :nb] != want[s][0])
        assert bad.size == 0, f"{tag}: stream {s}: bytes differ first at {bad[0]} of {len(bad)}"
        assert np.all(rows[s, nb:] == poison), f"{tag}: stream {s}: wrote past ceil(n_bits/8) bytes of its row"
        if want_n % 8:
            assert rows[s, nb - 1] & ((1 << (8 - want_n % 8)) - 1) == 0, f"{tag}: pad bits set"
    # the same data, one stream per call (of many streams the first two and the last)
    for s in range(ns) if ns <= 4 else (0, 1, ns - 1):
        one, n_one = dec.decode_stream(d_buf[s * pitch:s * pitch + T], bool(flags & BEGIN), bool(flags & END), W, head, tail)
        assert n_one == want_n and np.array_equal(one.cpu().numpy(), rows[s, :nb]), (tag, s)
    return rows[:, :nb]


def run_cases(oracle, code, decode_type, dec, ebn0, seed, cases):
    pc, _, _ = make_table_config(code, decode_type)
    longest = max(c[1] for c in cases) + 40
    most = max(c[0] for c in cases)
    # a few independent noisy streams, handed out in turn with different offsets
    pool = [make_stream(code, pc, longest + 64, ebn0, seed + j)[1] for j in range(min(most, 4))]
    for k, (ns, T, W, head, tail, flags, extra) in enumerate(cases):
        pitch = (-(-T // W) + extra) * W
        assert streams_windows(code.K, ns, pitch, T, W, head, tail, flags)
        streams = []
        for s in range(ns):
            first = 0 if flags & BEGIN else 5 + (s * 7 + k) % 50
            streams.append(pool[s % len(pool)][first:first + T])
            assert streams[-1].shape[0] == T
        decode_and_compare(oracle, code, decode_type, dec, streams, pitch, W, head, tail, flags, extra_out=(0, 5, 16, 29)[k % 4])


STOCK_SETS = [(COMMON_CODES[2], t) for t in DECODE_TYPES] + [
    (COMMON_CODES[0], "SOFT16"), (COMMON_CODES[1], "SOFT8"), (COMMON_CODES[3], "SOFT8"), (COMMON_CODES[4], "SOFT16"),
    (COMMON_CODES[5], "SOFT16"), (COMMON_CODES[6], "SOFT8")]


@pytest.mark.parametrize("code,decode_type", STOCK_SETS, ids=lambda x: getattr(x, "name", x))
def test_register_plan_bit_exact(oracle, code, decode_type):
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    assert dec.plan == _lib.PLAN_REG
    tile = dec._handle.info.workspace_tile_frames
    run_cases(oracle, code, decode_type, dec, 3.0, seed=code.K * 10 + code.R, cases=grid_cases(code.K, tile))


def test_generic_kernels_bit_exact(oracle, monkeypatch, tmp_path):
    _no_compiler(monkeypatch, tmp_path)
    code = Code("custom K7", 7, 2, (0o147, 0o135))
    for decode_type in ("SOFT16", "SOFT8"):
        pc, table, config = make_table_config(code, decode_type)
        dec = BatchDecoder(table, config)
        assert dec.plan == _lib.PLAN_REG and "GENERIC" in dec.plan_note, dec.plan_note
        run_cases(oracle, code, decode_type, dec, 3.0, seed=5, cases=grid_cases(code.K, dec._handle.info.workspace_tile_frames))


@pytest.mark.parametrize("code,decode_type", [(Code("K10", 10, 2, (0o1473, 0o1051)), "SOFT16"), (Code("K10", 10, 2, (0o1473, 0o1051)), "SOFT8"),
                                              (COMMON_CODES[7], "SOFT16"), (COMMON_CODES[7], "SOFT8")],
                         ids=["K10-16", "K10-8", "K15-16", "K15-8"])
def test_lds2_bit_exact(oracle, code, decode_type):
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    assert dec.plan == _lib.PLAN_LDS2
    K, d, m = code.K, default_extension(code.K), code.K - 1
    Wd = max(64, d)
    # PLAN_LDS2 works on frame pairs: a "tile" of 2.  K = 15 costs the CPU checker 16384 states a step: fewer and shorter cases
    cases = grid_cases(K, 2) if K == 10 else [
        (2, d + 2 * Wd + d, Wd, d, d, BEGIN, 0), (3, d + Wd + d + 21, Wd, d, d, END, 1), (3, m + 3 * (m + 3) + m, m + 3, m, m, END, 0),
        (2, d + d + 9, Wd, d, d, BEGIN | END, 0), (3, (m + 1) + 2 * (m + 7) + (m + 2) + 3, m + 7, m + 1, m + 2, 0, 0)]
    run_cases(oracle, code, decode_type, dec, 3.0 if K == 10 else -2.0, seed=K, cases=cases)


@pytest.mark.parametrize("code,decode_type", [(COMMON_CODES[2], "SOFT16"), (COMMON_CODES[3], "SOFT8"), (Code("K2", 2, 2, (0o3, 0o1)), "SOFT8")],
                         ids=["Voyager-16", "LTE-8", "K2-8"])
def test_plan_lds_forced_bit_exact(oracle, code, decode_type):
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config, plan=_lib.PLAN_LDS)
    assert dec.plan == _lib.PLAN_LDS
    run_cases(oracle, code, decode_type, dec, 3.0, seed=code.K + 3, cases=grid_cases(code.K, 8))


def test_python_layer_and_padding_independence(oracle):
    """BatchDecoder.decode_streams on a [n_streams][pitch][R] tensor: the rows, an `out` with wider rows, and the same bytes
    whatever the padding holds"""
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    ocfg = oracle_cfg("SOFT16", code.R)
    dec = BatchDecoder(table, config)
    W, head, tail, ns = 128, 48, 48, 4
    T = head + 6 * W + tail
    pitch = 8 * W
    streams = [make_stream(code, pc, T, 2.5, seed=60 + s)[1][:T] for s in range(ns)]
    want = np.stack([stream_reference(oracle, code, ocfg, s, W, head, tail, BEGIN)[0] for s in streams])
    results = []
    for fill in (0, 1234, -777):
        buf = np.full((ns, pitch, code.R), fill, dtype=np.int16)
        for s in range(ns):
            buf[s, :T] = streams[s]
        got, n = dec.decode_streams(torch.from_numpy(buf).cuda(), steps=T, begin=True, end=False, window=W, head=head, tail=tail)
        assert n == T - tail and tuple(got.shape) == (ns, (n + 7) // 8)
        results.append(got.cpu().numpy())
        assert np.array_equal(results[-1], want)
    wide = torch.full((ns, want.shape[1] + 9), 0x5A, dtype=torch.uint8, device="cuda")
    got, n = dec.decode_streams(torch.from_numpy(buf).cuda(), steps=T, window=W, head=head, tail=tail, out=wide)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want) and torch.all(wide[:, want.shape[1]:] == 0x5A)
    with pytest.raises(ValueError):
        dec.decode_streams(torch.from_numpy(buf).cuda()[:, :pitch - 1].contiguous(), steps=T, window=W, head=head, tail=tail)   # pitch % W


def test_argument_and_workspace_errors():
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    lib, h = _lib.load(), dec._handle._h
    ns, T, W = 3, 5000, 64
    pitch = 79 * W
    nb = (T - 6 + 7) // 8
    sym = torch.zeros((ns, pitch, code.R), dtype=torch.int16, device="cuda")
    need = lib.vit_hip_streams_workspace_bytes(h, ns, pitch, T, W, 6, 6, BEGIN)
    assert need > 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    out = torch.full((ns * (nb + 8) + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    n_bits = C.c_size_t(777)

    def call(symbols=p(sym), ns=ns, pitch=pitch, T=T, W=W, head=6, tail=6, flags=BEGIN, workspace=p(ws), nbytes=need, out_ptr=p(out),
             out_pitch=nb + 8):
        return lib.vit_hip_decode_streams(h, symbols, ns, pitch, T, W, head, tail, flags, workspace, nbytes, out_ptr, out_pitch,
                                          C.byref(n_bits), None)

    rejected = (dict(pitch=pitch + 1), dict(pitch=T), dict(pitch=78 * W), dict(pitch=T - 1), dict(ns=0), dict(out_pitch=nb - 1), dict(out_pitch=0),
                # what vit_hip_decode_stream rejects
                dict(head=5), dict(tail=5), dict(W=7, pitch=7 * 715), dict(W=40, head=41, pitch=40 * 125), dict(W=40, tail=41, pitch=40 * 125),
                dict(flags=4), dict(flags=BEGIN | 8), dict(T=11), dict(T=12, flags=0), dict(T=12, flags=END), dict(T=1 << 31, pitch=1 << 31),
                dict(ns=1 << 31),
                dict(symbols=None), dict(workspace=None), dict(out_ptr=None), dict(symbols=C.c_void_p(sym.data_ptr() + 1)))
    for kwargs in rejected:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG, kwargs
        a = {k: v for k, v in kwargs.items() if k in ("ns", "pitch", "T", "W", "head", "tail", "flags")}
        if a:
            full = dict(dict(ns=ns, pitch=pitch, T=T, W=W, head=6, tail=6, flags=BEGIN), **a)
            assert lib.vit_hip_streams_workspace_bytes(h, full["ns"], full["pitch"], full["T"], full["W"], full["head"], full["tail"],
                                                       full["flags"]) == 0, kwargs
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(workspace=C.c_void_p(ws.data_ptr() + 16)) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.all(out == 0xAB) and n_bits.value == 777, "a rejected call wrote its outputs"
    with pytest.raises(ValueError):
        dec.decode_streams(sym, steps=T, window=W, head=3, tail=6)
    assert call() == _lib.OK and n_bits.value == T - 6                        # the same buffers are fine
    assert call(out_pitch=nb) == _lib.OK
    assert lib.vit_hip_decode_streams(h, p(sym), ns, pitch, T, W, 6, 6, BEGIN, p(ws), need, p(out), nb, None, None) == _lib.OK
    torch.cuda.synchronize()


def test_graph_capture_and_two_calls_in_flight(oracle):
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    ocfg = oracle_cfg("SOFT16", code.R)
    dec = BatchDecoder(table, config)
    W, head, tail, ns = 128, 48, 48, 5
    shapes = [(head + 12 * W + tail + 77, True, True), (head + 9 * W + tail, False, False)]      # 8 launches; 5 launches

    def make(T, seed):
        pitch = -(-T // W) * W
        buf = np.zeros((ns, pitch, code.R), dtype=np.int16)
        syms = [make_stream(code, pc, T, 2.5, seed=seed + s)[1][:T] for s in range(ns)]
        for s in range(ns):
            buf[s, :T] = syms[s]
        return buf, syms

    def reference(syms, b, e):
        return np.stack([stream_reference(oracle, code, ocfg, s, W, head, tail, (BEGIN if b else 0) | (END if e else 0))[0] for s in syms])

    bufs, wants, wss, outs = [], [], [], []
    for k, (T, b, e) in enumerate(shapes):
        buf, syms = make(T, 300 + 10 * k)
        bufs.append(torch.from_numpy(buf).cuda())
        wants.append(reference(syms, b, e))
        wss.append(torch.empty(dec.streams_workspace_bytes(ns, buf.shape[1], T, b, e, W, head, tail), dtype=torch.uint8, device="cuda"))
        outs.append(torch.zeros(wants[-1].shape, dtype=torch.uint8, device="cuda"))
    # two calls on two HIP streams of one handle, each with its own workspace
    hip_streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for st, d, (T, b, e), o, w in zip(hip_streams, bufs, shapes, outs, wss):
        with torch.cuda.stream(st):
            dec.decode_streams(d, T, b, e, W, head, tail, out=o, workspace=w)
    torch.cuda.synchronize()
    for o, want in zip(outs, wants):
        assert np.array_equal(o.cpu().numpy(), want)
    # each shape captured into a graph on a single stream, replayed on new symbols
    for k, (T, b, e) in enumerate(shapes):
        d, o, w = bufs[k], outs[k], wss[k]
        dec.decode_streams(d, T, b, e, W, head, tail, out=o, workspace=w)               # warm-up outside capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            dec.decode_streams(d, T, b, e, W, head, tail, out=o, workspace=w)
        for seed in (400, 500):
            buf, syms = make(T, seed + 10 * k)
            d.copy_(torch.from_numpy(buf))
            o.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(o.cpu().numpy(), reference(syms, b, e)), (k, seed)


@pytest.mark.parametrize("code_id,decode_type,W,head,tail,ns", [(2, "SOFT16", 128, None, None, 3), (3, "SOFT8", 67, 9, 13, 2), (5, "SOFT16", 256, None, None, 5)])
def test_multi_stream_decoder_ragged_pushes(code_id, decode_type, W, head, tail, ns):
    """pushes of random ragged sizes, the same for all streams (they run in lockstep), plus finish(): per stream the bytes of ONE
    decode_stream call over that whole stream, and every internal call a uniform segment on the window grid"""
    import torch

    code = COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    rng = np.random.default_rng(code_id + 70)
    hd = default_extension(code.K) if head is None else head
    tl = default_extension(code.K) if tail is None else tail
    for trial, L in enumerate((30 * W + 5, 11 * W + 3, hd + tl + 40)):
        syms = np.stack([make_stream(code, pc, L, 3.0, seed=trial * 10 + s + 5)[1] for s in range(ns)])
        T = syms.shape[1]
        d_sym = torch.from_numpy(syms).cuda()
        md = MultiStreamDecoder(dec, ns, W, head, tail)
        data, pos = [b""] * ns, 0
        while pos < T:
            n = int(min(T - pos, rng.integers(1, 5 * W)))
            last = pos + n == T
            part = md.finish(d_sym[:, pos:pos + n]) if last and trial % 2 == 0 else md.push(d_sym[:, pos:pos + n])
            assert len(part) == ns and len({len(x) for x in part}) == 1
            data = [x + y for x, y in zip(data, part)]
            pos += n
        if not md._done:
            data = [x + y for x, y in zip(data, md.finish())]
        assert md.n_bits == L
        for s in range(ns):
            one, n_one = dec.decode_stream(d_sym[s].contiguous(), True, True, W, head, tail)
            assert n_one == L and len(data[s]) == (L + 7) // 8
            assert np.array_equal(np.frombuffer(data[s], dtype=np.uint8), one.cpu().numpy()), (code.name, trial, s, md.calls)
        for steps, begin, end in md.calls:
            assert end or (steps - hd - tl) % W == 0, "internal calls are uniform batches"
        assert [c[1] for c in md.calls] == [True] + [False] * (len(md.calls) - 1) and md.calls[-1][2]
        if trial == 0:
            assert len(md.calls) > 2


def _best_of_three(fn, iters):
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


# K = 7 R = 1/2 SOFT16, W = 1024 at the default extension, 64 streams of 16 windows each (T = 48 + 16 * 1024 + 48, pitch 17 * 1024).
# (a) against what one stream per call offers for the same job, 64 back-to-back vit_hip_decode_stream calls on one HIP stream: the
#     one call must not be slower (ratio <= 1.0) -- the reason the feature exists, not a tuned number.
# (b) against ONE vit_hip_decode_stream over a single stream holding the same 64 * 16 useful windows: time of the new call / time of
#     that call, measured on one MI355X (profiles/streams_rate.txt); the bound is that x 1.15, the margin for the box-to-box spread
#     tests/test_gpu_stream.py uses.  Measured: 0.325 ms for the new call, 20.2 ms for (a) (ratio 0.016), 0.325 ms for (b) (ratio
#     0.998 and 0.999 in two runs).  The grid carries m / n = 17 / 16 of the windows, but at a thousand windows both calls of (b) last
#     as long as ONE window's dependent chain, so the bridge windows cost nothing yet (profiles/streams_summary.md).
MEASURED_RATIO = 0.999
RATIO_BOUND = MEASURED_RATIO * 1.15


def test_streams_rate_against_one_stream_per_call():
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    lib, h = _lib.load(), dec._handle._h
    W, head, tail, ns, n = 1024, 48, 48, 64, 16
    T = head + n * W + tail
    pitch = (n + 1) * W
    T_one = head + ns * n * W + tail                                # one stream with the same useful windows
    _, sym = make_stream(code, pc, 1 << 16, 3.0, seed=2)
    steps = max(ns * pitch, T_one)
    d_sym = torch.from_numpy(sym[:1 << 16]).cuda().repeat(steps // (1 << 16) + 1, 1)[:steps].contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    step_bytes = code.R * 2
    need_all = lib.vit_hip_streams_workspace_bytes(h, ns, pitch, T, W, head, tail, BEGIN)
    need_each = lib.vit_hip_stream_workspace_bytes(h, T, W, head, tail, BEGIN)
    need_one = lib.vit_hip_stream_workspace_bytes(h, T_one, W, head, tail, BEGIN)
    assert min(need_all, need_each, need_one) > 0
    ws = torch.empty(max(need_all, need_each, need_one), dtype=torch.uint8, device="cuda")
    nb = (T - tail + 7) // 8
    out = torch.empty((ns, nb), dtype=torch.uint8, device="cuda")
    out_each = torch.empty((ns, nb), dtype=torch.uint8, device="cuda")
    out_one = torch.empty((T_one - tail + 7) // 8, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def streams():
        assert lib.vit_hip_decode_streams(h, p(d_sym), ns, pitch, T, W, head, tail, BEGIN, p(ws), need_all, p(out), nb, None, st) == _lib.OK

    def per_call():
        for s in range(ns):
            assert lib.vit_hip_decode_stream(h, C.c_void_p(d_sym.data_ptr() + s * pitch * step_bytes), T, W, head, tail, BEGIN, p(ws), need_each,
                                             C.c_void_p(out_each.data_ptr() + s * nb), None, st) == _lib.OK

    def one_stream():
        assert lib.vit_hip_decode_stream(h, p(d_sym), T_one, W, head, tail, BEGIN, p(ws), need_one, p(out_one), None, st) == _lib.OK

    per_call(), streams()
    torch.cuda.synchronize()
    assert torch.equal(out, out_each), "the one call and the 64 calls decode the same bytes"
    one_stream()
    t_streams, t_calls, t_one = _best_of_three(streams, 20), _best_of_three(per_call, 3), _best_of_three(one_stream, 20)
    gbit = ns * (T - tail) / t_streams / 1e9
    print(f"streams {t_streams * 1e3:.3f} ms ({gbit:.1f} Gbit/s emitted), {ns} calls of one stream {t_calls * 1e3:.3f} ms "
          f"(ratio {t_streams / t_calls:.4f}, bound 1.0), one stream of {ns * n} windows {t_one * 1e3:.3f} ms "
          f"(ratio {t_streams / t_one:.3f}, measured {MEASURED_RATIO}, bound {RATIO_BOUND})")
    assert t_streams <= 1.0 * t_calls, (t_streams, t_calls)
    assert t_streams <= RATIO_BOUND * t_one, (t_streams, t_one)
