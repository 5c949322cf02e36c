"""One long stream decoded as overlapped windows (vit_hip_decode_stream) against its restatement on the CPU checker
(tests/stream_reference.py): bit for bit on every plan, n_bits and pad bits, argument errors, concurrency, graph capture,
StreamDecoder, the punctured composition and the cost against the plain decode of the same trellis work."""
import ctypes as C
import time

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, BatchDecoder, Code, StreamDecoder, _lib
from tests.helpers import DECODE_TYPES, make_table_config, oracle_cfg
from tests.stream_reference import BEGIN, END, default_extension, make_stream, stream_reference, stream_windows

pytestmark = pytest.mark.gpu


def _no_compiler(monkeypatch, tmp_path):
    """as tests/test_gpu_generic.py: no hipcc and an empty user cache, so a code outside the stock table runs the GENERIC kernels"""
    monkeypatch.setenv("VIT_HIP_HIPCC", "/nonexistent/hipcc")
    monkeypatch.setenv("VIT_HIP_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("VIT_HIP_JIT", raising=False)


def shape_cases(K, tile):
    """(T, W, head, tail, flags).  All four flag combinations; uniform-only shapes (T = head + n W + tail without END) and shapes
    with the longer last window; n = 1; W, head, tail odd and at their minima (W = max(8, K-1), head = tail = K-1); window counts
    that leave a partial tile and that go beyond one tile of `tile` frames."""
    d = default_extension(K)
    m = K - 1
    Wmin = max(8, m)
    Wd = max(64, d)                       # a small window that admits the default extension
    big = tile + tile // 2 + 3            # windows: more than one tile, the last one partial
    return [
        (d + 5 * Wd + d, Wd, d, d, BEGIN),                              # uniform, 5 windows (a partial tile)
        (d + 5 * Wd + d, Wd, d, d, 0),
        (d + 5 * Wd + d + 37, Wd, d, d, BEGIN | END),                   # remainder window, END
        (d + 4 * Wd + d + 11, Wd, d, d, END),
        (d + 3 * Wd + d + 29, Wd, d, d, 0),                             # remainder window without END: its own end-state select
        (d + Wd + d, Wd, d, d, BEGIN),                                  # n = 1, uniform
        (d + d + 9, Wd, d, d, BEGIN | END),                             # n = 1, shorter than a window
        (m + m + 1, Wmin, m, m, 0),                                     # the least of everything: one bit out
        (m + big * Wmin + m, Wmin, m, m, BEGIN),                        # the minima, uniform, beyond one tile
        (m + big * Wmin + m + 5, Wmin, m, m, END),
        ((m + 2) + 7 * (Wmin + 5) + (m + 4) + 3, Wmin + 5, m + 2, m + 4, BEGIN | END),   # odd W / head / tail
        ((m + 3) + big * (Wmin + 9) + m, Wmin + 9, m + 3, m, 0),
        # under END the last window is uniform exactly when the remainder r + K-1 equals tail
        (d + 6 * Wd + d, Wd, d, d, BEGIN | END) if d > m else (m + 6 * Wmin + m, Wmin, m, m, BEGIN | END),
    ]


def decode_and_compare(oracle, code, decode_type, dec, sym, W, head, tail, flags, poison=0xA5):
    """one call on poisoned buffers against the restatement; returns the decoded bits"""
    import torch

    T = sym.shape[0]
    d_sym = torch.from_numpy(np.ascontiguousarray(sym)).cuda()
    need = dec.stream_workspace_bytes(T, bool(flags & BEGIN), bool(flags & END), W, head, tail)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need,), poison, dtype=torch.uint8, device="cuda")
    want, want_n = stream_reference(oracle, code, oracle_cfg(decode_type, code.R), sym, W, head, tail, flags)
    out = torch.full((want.size + 32,), poison, dtype=torch.uint8, device="cuda")
    off = T % 2                                                    # every other shape writes an output that is not 16-byte aligned
    got, n = dec.decode_stream(d_sym, bool(flags & BEGIN), bool(flags & END), W, head, tail, out=out[off:off + want.size], workspace=ws)
    torch.cuda.synchronize()
    tag = (code.name, decode_type, T, W, head, tail, flags, _lib.PLAN_NAMES[dec.plan])
    assert n == want_n, tag
    host = out.cpu().numpy()
    assert np.all(host[:off] == poison), f"{tag}: wrote in front of the output"
    host = host[off:]
    bad = np.argwhere(host[:want.size] != want)
    assert bad.size == 0, f"{tag}: bytes differ first at {bad[0]} of {len(bad)}"
    assert np.all(host[want.size:] == poison), f"{tag}: wrote past ceil(n_bits/8) bytes"
    if n % 8:
        assert host[want.size - 1] & ((1 << (8 - n % 8)) - 1) == 0, f"{tag}: pad bits set"
    return np.unpackbits(host[:want.size])[:n]


def run_cases(oracle, code, decode_type, dec, ebn0, seed, cases=None):
    pc, _, _ = make_table_config(code, decode_type)
    tile = dec._handle.info.workspace_tile_frames
    cases = shape_cases(code.K, tile) if cases is None else cases
    longest = max(c[0] for c in cases) + 40
    _, stream = make_stream(code, pc, longest, ebn0, seed)
    for k, (T, W, head, tail, flags) in enumerate(cases):
        # BEGIN segments start at the stream's start, the others mid-stream; END segments need not hold a real tail to be bit-exact
        first = 0 if flags & BEGIN else 17 + k
        sym = stream[first:first + T]
        assert sym.shape[0] == T
        decode_and_compare(oracle, code, decode_type, dec, sym, W, head, tail, flags)


STOCK_SETS = [(COMMON_CODES[2], t) for t in DECODE_TYPES] + [
    (COMMON_CODES[0], "SOFT16"), (COMMON_CODES[1], "SOFT8"), (COMMON_CODES[3], "SOFT8"), (COMMON_CODES[4], "SOFT16"),
    (COMMON_CODES[5], "SOFT16"), (COMMON_CODES[6], "SOFT8")]


@pytest.mark.parametrize("code,decode_type", STOCK_SETS, ids=lambda x: getattr(x, "name", x))
def test_register_plan_bit_exact(oracle, code, decode_type):
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    assert dec.plan == _lib.PLAN_REG
    run_cases(oracle, code, decode_type, dec, 3.0, seed=code.K * 10 + code.R)


def test_generic_kernels_bit_exact(oracle, monkeypatch, tmp_path):
    _no_compiler(monkeypatch, tmp_path)
    code = Code("custom K7", 7, 2, (0o147, 0o135))
    for decode_type in ("SOFT16", "SOFT8"):
        pc, table, config = make_table_config(code, decode_type)
        dec = BatchDecoder(table, config)
        assert dec.plan == _lib.PLAN_REG and "GENERIC" in dec.plan_note, dec.plan_note
        run_cases(oracle, code, decode_type, dec, 3.0, seed=5)


@pytest.mark.parametrize("code,decode_type", [(Code("K10", 10, 2, (0o1473, 0o1051)), "SOFT16"), (Code("K10", 10, 2, (0o1473, 0o1051)), "SOFT8"),
                                              (COMMON_CODES[7], "SOFT16"), (COMMON_CODES[7], "SOFT8")],
                         ids=["K10-16", "K10-8", "K15-16", "K15-8"])
def test_lds2_bit_exact(oracle, code, decode_type):
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config)
    assert dec.plan == _lib.PLAN_LDS2
    K, d, m = code.K, default_extension(code.K), code.K - 1
    Wd = max(64, d)
    cases = shape_cases(K, 2) if K == 10 else [
        (d + 3 * Wd + d, Wd, d, d, BEGIN), (d + 2 * Wd + d + 21, Wd, d, d, END), (m + 3 * (m + 3) + m + 5, m + 3, m, m, 0),
        (d + d + 9, Wd, d, d, BEGIN | END), ((m + 1) + 2 * (m + 7) + (m + 2) + 3, m + 7, m + 1, m + 2, BEGIN | END)]
    run_cases(oracle, code, decode_type, dec, 3.0 if K == 10 else -2.0, seed=K, cases=cases)


@pytest.mark.parametrize("code,decode_type", [(COMMON_CODES[2], "SOFT16"), (COMMON_CODES[3], "SOFT8"), (Code("K2", 2, 2, (0o3, 0o1)), "SOFT8")],
                         ids=["Voyager-16", "LTE-8", "K2-8"])
def test_plan_lds_forced_bit_exact(oracle, code, decode_type):
    pc, table, config = make_table_config(code, decode_type)
    dec = BatchDecoder(table, config, plan=_lib.PLAN_LDS)
    assert dec.plan == _lib.PLAN_LDS
    run_cases(oracle, code, decode_type, dec, 3.0, seed=code.K + 3, cases=shape_cases(code.K, 8))


def test_noise_free_stream_round_trip(oracle):
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    L = 20000 + 3
    bits, sym = make_stream(code, pc, L, None, seed=9)
    got = decode_and_compare(oracle, code, "SOFT16", dec, sym, 1024, 48, 48, BEGIN | END)
    assert np.array_equal(got, bits)


def test_argument_and_workspace_errors():
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    lib, h = _lib.load(), dec._handle._h
    T, W = 5000, 64
    sym = torch.zeros((T, code.R), dtype=torch.int16, device="cuda")
    need = lib.vit_hip_stream_workspace_bytes(h, T, W, 6, 6, BEGIN)
    assert need > 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    out = torch.full((T // 8 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    n_bits = C.c_size_t(777)

    def call(symbols=p(sym), T=T, W=W, head=6, tail=6, flags=BEGIN, workspace=p(ws), nbytes=need, out_ptr=p(out)):
        return lib.vit_hip_decode_stream(h, symbols, T, W, head, tail, flags, workspace, nbytes, out_ptr, C.byref(n_bits), None)

    rejected = (dict(head=5), dict(tail=5), dict(W=7), dict(W=40, head=41), dict(W=40, tail=41), dict(flags=4), dict(flags=BEGIN | 8),
                dict(T=11), dict(T=12, flags=0), dict(T=12, flags=END), dict(T=1 << 31), dict(W=1 << 29, head=6, tail=6),
                dict(symbols=None), dict(workspace=None), dict(out_ptr=None), dict(symbols=C.c_void_p(sym.data_ptr() + 1)))
    for kwargs in rejected:
        assert call(**kwargs) == _lib.ERR_INVALID_ARG, kwargs
        a = {k: v for k, v in kwargs.items() if k in ("T", "W", "head", "tail", "flags")}
        if a:
            full = dict(dict(T=T, W=W, head=6, tail=6, flags=BEGIN), **a)
            assert lib.vit_hip_stream_workspace_bytes(h, full["T"], full["W"], full["head"], full["tail"], full["flags"]) == 0, kwargs
    assert call(nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert call(workspace=C.c_void_p(ws.data_ptr() + 16)) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.all(out == 0xAB) and n_bits.value == 777, "a rejected call wrote its outputs"
    with pytest.raises(ValueError):
        dec.decode_stream(sym, head=3)
    assert lib.vit_hip_stream_workspace_bytes(h, 12, W, 6, 6, BEGIN) > 0 and call(T=12) == _lib.OK     # head bits out of head + tail steps
    assert n_bits.value == 6
    assert call() == _lib.OK and n_bits.value == T - 6                        # the same buffers are fine
    assert lib.vit_hip_decode_stream(h, p(sym), T, W, 6, 6, BEGIN, p(ws), need, p(out), None, None) == _lib.OK   # n_bits_out may be NULL
    torch.cuda.synchronize()


def test_two_streams_and_graph_capture(oracle):
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    ocfg = oracle_cfg("SOFT16", code.R)
    dec = BatchDecoder(table, config)
    W, head, tail = 128, 48, 48
    T = head + 40 * W + tail + 77
    _, sym = make_stream(code, pc, 2 * T, 2.5, seed=77)
    segs = [sym[:T], sym[T - 100:2 * T - 100]]
    flags = [(True, True), (False, False)]
    d_segs = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in segs]
    want = [stream_reference(oracle, code, ocfg, s, W, head, tail, (BEGIN if b else 0) | (END if e else 0)) for s, (b, e) in zip(segs, flags)]
    # two calls on two streams of one handle, each with its own workspace
    wss = [torch.empty(dec.stream_workspace_bytes(T, b, e, W, head, tail), dtype=torch.uint8, device="cuda") for b, e in flags]
    outs = [torch.empty(w[0].size, dtype=torch.uint8, device="cuda") for w in want]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for s, d, (b, e), o, w in zip(streams, d_segs, flags, outs, wss):
        with torch.cuda.stream(s):
            dec.decode_stream(d, b, e, W, head, tail, out=o, workspace=w)
    torch.cuda.synchronize()
    for o, (wb, _) in zip(outs, want):
        assert np.array_equal(o.cpu().numpy(), wb)
    # one call captured into a graph on a single stream, replayed twice on new symbols
    d_sym, out, ws = d_segs[0], outs[0], wss[0]
    dec.decode_stream(d_sym, True, True, W, head, tail, out=out, workspace=ws)          # warm-up outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec.decode_stream(d_sym, True, True, W, head, tail, out=out, workspace=ws)
    for seed in (78, 79):
        _, s2 = make_stream(code, pc, T, 2.5, seed=seed)
        s2 = s2[:T]
        d_sym.copy_(torch.from_numpy(np.ascontiguousarray(s2)))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        wb, _ = stream_reference(oracle, code, ocfg, s2, W, head, tail, BEGIN | END)
        assert np.array_equal(out.cpu().numpy(), wb)


@pytest.mark.parametrize("code_id,decode_type,W,head,tail", [(2, "SOFT16", 128, None, None), (3, "SOFT8", 67, 9, 13), (5, "SOFT16", 256, None, None)])
def test_stream_decoder_ragged_pushes(oracle, code_id, decode_type, W, head, tail):
    """pushes of random ragged sizes plus finish(): every internal call is a segment on the window grid and the final segment holds
    a full window (StreamDecoder holds one back), so the result equals ONE decode_stream call over the concatenated stream -- and
    each internal call equals the restatement of that segment"""
    import torch

    code = COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    ocfg = oracle_cfg(decode_type, code.R)
    dec = BatchDecoder(table, config)
    rng = np.random.default_rng(code_id + 40)
    hd = default_extension(code.K) if head is None else head
    tl = default_extension(code.K) if tail is None else tail
    for trial, L in enumerate((30 * W + 5, 11 * W + 3, hd + tl + 40)):
        bits, sym = make_stream(code, pc, L, 3.0, seed=trial + 5)
        T = sym.shape[0]
        d_sym = torch.from_numpy(sym).cuda()
        sd = StreamDecoder(dec, W, head, tail)
        data, pos = b"", 0
        while pos < T:
            n = int(min(T - pos, rng.integers(1, 5 * W)))
            last = pos + n == T
            if last and trial % 2 == 0:
                data += sd.finish(d_sym[pos:pos + n])
            else:
                data += sd.push(d_sym[pos:pos + n])
            pos += n
        if not sd._done:
            data += sd.finish()
        assert sd.n_bits == L and len(data) == (L + 7) // 8
        one, n_one = dec.decode_stream(d_sym, True, True, W, head, tail)
        assert n_one == L
        assert np.array_equal(np.frombuffer(data, dtype=np.uint8), one.cpu().numpy()), (code.name, trial, sd.calls)
        # per internal call: the restatement of each segment, concatenated
        start, parts = 0, []
        for steps, begin, end in sd.calls:
            by, n = stream_reference(oracle, code, ocfg, sym[start:start + steps], W, hd, tl, (BEGIN if begin else 0) | (END if end else 0))
            parts.append(np.unpackbits(by)[:n])
            assert end or (steps - hd - tl) % W == 0, "internal calls are uniform batches"
            start += steps - hd - tl
        assert np.array_equal(np.concatenate(parts), np.unpackbits(np.frombuffer(data, dtype=np.uint8))[:L])
        if trial == 0:
            assert len(sd.calls) > 2


def test_stream_decoder_input_forms(oracle):
    """push() / finish() take flat tensors, [n][R] tensors and [n][R] views that are not contiguous; every form passes through the
    receiver's pitched buffer.  First a piece under one window, then one of several windows (the buffer grows while steps are
    pending), then pieces whose step counts are no multiples of 8; the L % 8 = 5 last bits leave through the carry at finish()"""
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    W, head, tail, L = 64, 48, 48, 20 * 64 + 5
    bits, sym = make_stream(code, pc, L, 3.0, seed=31)
    T = sym.shape[0]
    d_sym = torch.from_numpy(sym).cuda()

    def spaced(x):                                     # every other row of a tensor twice as long
        wide = torch.full((2 * x.shape[0], code.R), 0x55, dtype=x.dtype, device=x.device)
        wide[::2] = x
        return wide[::2]

    forms = (lambda x: x.reshape(-1), lambda x: x, spaced)
    sizes = [40, 300, 131, 203, 77, 333]
    sizes.append(T - sum(sizes))
    assert sizes[0] < W and sizes[1] > 4 * W and sizes[-1] > 0 and all(n % 8 for n in sizes[2:])
    sd = StreamDecoder(dec, W, head, tail)
    data, pos = b"", 0
    for k, n in enumerate(sizes):
        piece = forms[k % 3](d_sym[pos:pos + n])
        assert piece.is_contiguous() == (k % 3 != 2)
        data += sd.finish(piece) if k == len(sizes) - 1 else sd.push(piece)
        if k == 0:
            assert data == b""
        pos += n
    assert sd.n_bits == L and isinstance(sd.n_bits, int) and len(data) == (L + 7) // 8
    one, n_one = dec.decode_stream(d_sym, True, True, W, head, tail)
    assert n_one == L and data == one.cpu().numpy().tobytes()
    want, want_n = stream_reference(oracle, code, oracle_cfg("SOFT16", code.R), sym, W, head, tail, BEGIN | END)
    assert want_n == L and data == want.tobytes(), sd.calls


def test_punctured_stream_composition(oracle):
    """K = 7 R = 1/2 punctured to 3/4 (mask 1 1 0 1 1 0 over three steps), depunctured by vit_hip_depuncture_batch with frames =
    the number of puncturing periods into the contiguous [T][R] stream, then decoded: bit-exact against the restatement on the
    depunctured symbols, and error-free on a noise-free stream"""
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    mask = np.array([1, 1, 0, 1, 1, 0], dtype=bool)
    periods = 4000
    L = 3 * periods - (code.K - 1)
    for ebn0 in (None, 5.0):
        bits, sym = make_stream(code, pc, L, ebn0, seed=3)
        flat = sym.reshape(periods, 6)
        sent = np.ascontiguousarray(flat[:, mask])                  # [periods][4]: what was transmitted
        dep = dec.depuncture(torch.from_numpy(sent).cuda(), mask)   # [periods][3][R] = [T][R], erasures 0
        torch.cuda.synchronize()
        dep_host = dep.cpu().numpy().reshape(-1, code.R)
        want_dep = np.where(mask[None, :], flat, 0).reshape(-1, code.R)
        assert np.array_equal(dep_host, want_dep)
        got = decode_and_compare(oracle, code, "SOFT16", dec, dep_host, 512, 96, 96, BEGIN | END)
        if ebn0 is None:
            assert np.array_equal(got, bits)


def _best_of_three(fn, iters=5):
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


# time of vit_hip_decode_stream / time of vit_hip_decode_batch over the same number of terminated frames of head + W + tail - (K-1)
# bits, K = 7 R = 1/2 SOFT16, one stream of 2^26 steps, W = 1024 at the default extension.  Measured on one MI355X
# (profiles/stream_rate.txt): 1.074 (0.586 ms against 0.545 ms); the bound is that x 1.15, the margin for the box-to-box spread the
# README records.  A side pass that regresses, or a gather that creeps in, fails here.
MEASURED_RATIO = 1.074
RATIO_BOUND = MEASURED_RATIO * 1.15


def test_stream_rate_against_plain_decode():
    import torch

    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    dec = BatchDecoder(table, config)
    W, head, tail = 1024, 48, 48
    n = (1 << 26) // W - 1
    T = head + n * W + tail                                        # one uniform batch
    _, sym = make_stream(code, pc, 1 << 16, 3.0, seed=2)
    d_sym = torch.from_numpy(sym[:1 << 16]).cuda().repeat(T // (1 << 16) + 1, 1)[:T].contiguous()
    ws = torch.empty(dec.stream_workspace_bytes(T, True, False, W, head, tail), dtype=torch.uint8, device="cuda")
    out = torch.empty((T - tail + 7) // 8, dtype=torch.uint8, device="cuda")
    Lf = head + W + tail - (code.K - 1)
    frames = d_sym[:1 << 16].repeat(n * (Lf + code.K - 1) // (1 << 16) + 1, 1)[:n * (Lf + code.K - 1)].reshape(n, Lf + code.K - 1, code.R).contiguous()
    fout = torch.empty((n, (Lf + 7) // 8), dtype=torch.uint8, device="cuda")

    def stream():
        dec.decode_stream(d_sym, True, False, W, head, tail, out=out, workspace=ws)

    def plain():
        dec.decode(frames, Lf, out=fout)

    plain(), stream()
    t_plain, t_stream = _best_of_three(plain), _best_of_three(stream)
    gbit = (T - tail) / t_stream / 1e9
    print(f"stream {t_stream * 1e3:.3f} ms ({gbit:.1f} Gbit/s emitted), plain decode of {n} frames x {Lf} bits {t_plain * 1e3:.3f} ms, "
          f"ratio {t_stream / t_plain:.3f} (measured {MEASURED_RATIO}, bound {RATIO_BOUND})")
    assert t_stream <= RATIO_BOUND * t_plain, (t_stream, t_plain)
