"""vit_hip_marker_search on the device against tests/marker_reference.py: distance, count and lock EQUAL to the numpy rule for every
marker length, shape, period, row layout and history the rule tells apart, both accumulate modes, planted markers, the call captured
into a graph, every rejection with the outputs untouched, the receivers' running totals, and the chain sync_search -> sync_build ->
decode_stream -> marker_search on an inverted Voyager stream."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import CCSDS_ASM, COMMON_CODES, DVB_SYNC, BatchDecoder, MultiStreamDecoder, StreamDecoder, _lib, frame_sync, synth
from viterbidecodercpp_amd.sync import NEG_EVEN, NEG_ODD, enumerate_hypotheses
from tests import marker_reference as mr
from tests import stream_reference as sr
from tests import sync_reference as sref
from tests.helpers import make_table_config, oracle_cfg

pytestmark = pytest.mark.gpu

POISON, GUARD = 0x5A5A5A5A, 64
LENGTHS = [1, 7, 8, 9, 31, 32, 33, 63, 64]


@functools.lru_cache(maxsize=None)
def decoder():
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    return code, pc, BatchDecoder(table, config)


def device_rows(c, off):
    """the case's rows on the device, the first `off` bytes into an allocation that ends with the last row's last byte"""
    import torch
    rows, stride, nb = c["rows"], c["stride"], c["nb"]
    flat = np.full(off + (rows - 1) * stride + max(nb, 1), 0xEE, dtype=np.uint8)
    for r in range(rows):
        flat[off + r * stride: off + r * stride + min(stride, flat.size - off - r * stride)] = c["bytes"][r, :min(stride, flat.size - off - r * stride)]
    d = torch.from_numpy(flat).cuda()
    return torch.as_strided(d, (rows, max(nb, 1)), (stride if rows > 1 else max(nb, 1), 1), off)


def guarded(rows, P):
    """(distance, count, lock) as slices of one poisoned buffer, and the check that nothing around them was written"""
    import torch
    sizes = [rows * P, rows * P, rows * 4]
    buf = torch.full((sum(sizes) + GUARD * (len(sizes) + 1),), POISON, dtype=torch.int32, device="cuda")
    outs, at = [], GUARD
    for n, shape in zip(sizes, [(rows, P), (rows, P), (rows, 4)]):
        outs.append(buf[at:at + n].view(shape))
        at += n + GUARD
    live = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    at = GUARD
    for n in sizes:
        live[at:at + n] = True
        at += n + GUARD
    return tuple(outs), lambda: bool((buf[~live] == POISON).all().item())


def as_u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def check(c, off=0, want=None):
    code, pc, dec = decoder()
    want = mr.case_reference(c) if want is None else want
    out, guards_ok = guarded(c["rows"], c["P"])
    d_bytes = device_rows(c, off)
    got = dec.marker_search(d_bytes, c["n_bits"], c["marker"], c["m"], c["P"], c["phase0"], c["history"], c["hb"], out=out)
    tag = {k: c[k] for k in ("rows", "n_bits", "m", "P", "hb", "phase0", "stride")} | {"off": off}
    for name, g, w in zip(("distance", "count", "lock"), got, want):
        g = as_u32(g)
        assert np.array_equal(g, w), (name, tag, np.argwhere(g != w)[:4].tolist())
    assert guards_ok(), tag
    return want


@pytest.mark.parametrize("m", LENGTHS)
def test_marker_lengths_shapes_and_periods(m):
    """one position, two, a row inside one tile, 4099 bits; every period class; rows 1 and 3 on and off 16 bytes, at strides of
    ceil(n_bits/8), +1 and +13"""
    i = 0
    for n_bits in (m, m + 1, 1000, 4099):
        for P in (1, max(m - 1, 1), 8, 13, 1632, n_bits + 5):
            if n_bits < m:
                continue
            c = mr.make_case(100 * m + i, rows=(1, 3)[i % 2], n_bits=n_bits, m=m, P=P, phase0=(0, 1, P - 1)[i % 3] % P,
                             stride_extra=(0, 1, 13)[(i // 2) % 3])
            check(c, off=(0, 1, 16, 5)[i % 4])
            i += 1


@pytest.mark.parametrize("marker,P", [(CCSDS_ASM, 1024), (CCSDS_ASM, 10232), (DVB_SYNC, 1632), (DVB_SYNC, 13056)])
def test_stock_markers(marker, P):
    c = mr.make_case(P, rows=3, n_bits=3 * P + 77, m=marker[1], P=P, marker=marker[0], hb=marker[1] - 1, phase0=P // 3, stride_extra=1,
                     plant=(P // 2, 0))
    want = check(c, off=3)
    assert (want[2][:, :3] == (P // 2, 0, 0)).all()


@pytest.mark.parametrize("rows,n_bits,m,P,extra", [
    (1, 200_003, 32, 64, 0),         # a phase's frames across 25 workgroups
    (3, 20_000, 32, 5000, 1),        # more phases than a workgroup has lanes; three tiles per workgroup
    (64, 1000, 8, 13, 13), (64, 1000, 33, 1632, 1),
    (64, 135_000, 8, 1632, 0),       # 64 x 17 tiles: two tiles per workgroup by the grid's size
    (2, 30_000, 9, 255, 0), (2, 30_000, 9, 256, 0), (2, 30_000, 9, 257, 0),          # sums in registers up to 256 phases
    (2, 60_000, 31, 12288, 0), (2, 60_000, 31, 12289, 5),                            # the LDS table up to 12288 phases
])
def test_larger_shapes_and_every_path(rows, n_bits, m, P, extra):
    c = mr.make_case(n_bits + P, rows=rows, n_bits=n_bits, m=m, P=P, hb=m - 1, phase0=P - 1, stride_extra=extra)
    check(c, off=extra)


@pytest.mark.parametrize("m", [8, 32, 64])
def test_history(m):
    i = 0
    for hb in (0, 1, m - 1, 63):
        for P in (13, 1):
            for phase0 in sorted({0, 1 % P, P - 1}):
                check(mr.make_case(7000 + 100 * m + i, rows=2, n_bits=1000, m=m, P=P, hb=hb, phase0=phase0), off=i % 3)
                i += 1
    # fewer bits than the marker, and none at all: every position starts in the history
    check(mr.make_case(1, rows=2, n_bits=m - 5, m=m, P=13, hb=63, phase0=4, stride_extra=2), off=1)
    check(mr.make_case(2, rows=1, n_bits=1, m=m, P=m + 5, hb=m - 1, phase0=3))
    check(mr.make_case(3, rows=3, n_bits=0 if m < 64 else 1, m=m, P=7, hb=63, phase0=6, stride_extra=1))    # m = 64 needs one bit
    if m < 64:
        check(mr.make_case(4, rows=1, n_bits=0, m=m, P=1, hb=m))


def test_two_accumulating_calls_equal_one():
    import torch
    code, pc, dec = decoder()
    c = mr.make_case(11, rows=3, n_bits=4099, m=32, P=13, hb=5, phase0=2, stride_extra=3)
    want = mr.case_reference(c)
    d_bytes = device_rows(c, 0)
    cut = 2048
    out, guards_ok = guarded(3, 13)
    for x in out:
        x.zero_()
    dec.marker_search(d_bytes, cut, c["marker"], 32, 13, 2, c["history"], 5, out=out, accumulate=True)
    history = [frame_sync.history_of(np.unpackbits(row)[:cut], 32)[0] for row in c["bytes"]]
    got = dec.marker_search(d_bytes[:, cut // 8:], 4099 - cut, c["marker"], 32, 13, (2 + cut) % 13, history, 31, out=out, accumulate=True)
    for g, w in zip(got, want):
        assert np.array_equal(as_u32(g), w)
    assert guards_ok()
    # a third accumulating call doubles nothing it should not: the totals grow by one call's worth
    again = dec.marker_search(d_bytes, 4099, c["marker"], 32, 13, 2, c["history"], 5, out=out, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(as_u32(again[0]), 2 * want[0]) and np.array_equal(as_u32(again[1]), 2 * want[1])
    assert np.array_equal(as_u32(again[2])[:, :2], want[2][:, :2])


@pytest.mark.parametrize("m,P,phase,inverted", [(32, 1024, 300, 0), (32, 1024, 1023, 1), (8, 1632, 0, 1), (64, 200, 77, 0), (7, 50, 49, 1)])
def test_planted_locks(m, P, phase, inverted):
    c = mr.make_case(m * P + phase, rows=2, n_bits=6 * P + 11, m=m, P=P, phase0=5 % P, plant=(phase, inverted))
    want = check(c)
    assert (want[2][:, :3] == (phase, inverted, 0)).all() and (want[2][:, 3] >= 5 * m).all()


def test_captured_into_a_graph_and_replayed():
    import torch
    code, pc, dec = decoder()
    cases = [mr.make_case(s, rows=2, n_bits=5000, m=32, P=1024, marker=CCSDS_ASM[0], hb=31, plant=(ph, inv))
             for s, ph, inv in ((21, 100, 0), (22, 900, 1))]
    d_bytes = device_rows(cases[0], 0)
    d_hist = torch.from_numpy(cases[0]["history"].view(np.int64)).cuda()
    out, guards_ok = guarded(2, 1024)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.marker_search(d_bytes, 5000, CCSDS_ASM[0], 32, 1024, 0, d_hist, 31, out=out)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec.marker_search(d_bytes, 5000, CCSDS_ASM[0], 32, 1024, 0, d_hist, 31, out=out)
    for c in cases:
        d_bytes.copy_(device_rows(c, 0))
        d_hist.copy_(torch.from_numpy(c["history"].view(np.int64)).cuda())
        for x in out:
            x.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, mr.case_reference(c)):
            assert np.array_equal(as_u32(g), w)
    assert guards_ok()


def test_rejections_launch_nothing():
    import torch
    code, pc, dec = decoder()
    lib, h = _lib.load(), dec._handle._h
    d_bytes = torch.zeros(256, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(2, dtype=torch.int64, device="cuda")
    out, guards_ok = guarded(2, 16)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def search(bytes=d_bytes, stride=0, rows=2, n_bits=1000, marker=0x47, m=8, history=None, hb=0, P=16, phase0=0, flags=0, distance=out[0],
               count=out[1], lock=out[2], handle=h):
        return lib.vit_hip_marker_search(handle, ptr(bytes), stride, rows, n_bits, marker, m, ptr(history), hb, P, phase0, flags, ptr(distance),
                                         ptr(count), ptr(lock), stream)

    rejected = {
        "NULL handle": search(handle=None), "NULL bytes": search(bytes=None), "NULL distance": search(distance=None),
        "accumulate: lock without count": search(flags=1, count=None),
        "m = 0": search(m=0, marker=0), "m = 65": search(m=65), "marker bits above m": search(marker=0x147), "bit 63 above m = 63": search(m=63, marker=1 << 63),
        "hb = 64": search(hb=64, history=d_hist), "history NULL with hb > 0": search(hb=3),
        "n_bits + hb < m": search(n_bits=4, hb=3, history=d_hist), "n_bits = 2^32 - 64": search(n_bits=(1 << 32) - 64, rows=1, P=1 << 30),
        "P = 0": search(P=0), "P = 2^31": search(P=1 << 31), "phase0 = P": search(phase0=16),
        "stride below the row": search(stride=124), "unknown flag bits": search(flags=2), "accumulate and unknown bits": search(flags=3),
        "a sum could wrap": search(n_bits=(1 << 27) + 8, m=64, marker=1, P=1, rows=1),
    }
    torch.cuda.synchronize()
    for what, rc in rejected.items():
        assert rc == _lib.ERR_INVALID_ARG, (what, rc)
    assert all((x == POISON).all().item() for x in out) and guards_ok()
    assert search(rows=0) == _lib.OK                                        # no work
    torch.cuda.synchronize()
    assert all((x == POISON).all().item() for x in out)
    assert search(stride=125, n_bits=1000, count=None) == _lib.OK          # the bounds are tight, and a passing call does write
    torch.cuda.synchronize()
    assert not (out[0] == POISON).any().item() and (out[1] == POISON).all().item() and guards_ok()
    assert search(n_bits=5, hb=3, history=d_hist, lock=None) == _lib.OK
    torch.cuda.synchronize()
    assert int(out[1].sum().item()) == 2 and guards_ok()                    # one position per row
    # the lock of a call without d_count: the counts of this call alone
    assert search(stride=125, n_bits=1000, count=None, phase0=3) == _lib.OK
    torch.cuda.synchronize()
    d, n = mr.search_fast(np.zeros((2, 125), dtype=np.uint8), 1000, 0x47, 8, 16, 3)
    assert np.array_equal(as_u32(out[0]), d) and np.array_equal(as_u32(out[2]), mr.pick(d, n, 8))
    with pytest.raises(_lib.VitHipError):
        dec.marker_search(d_bytes, 1000, 0x147, 8, 16)
    with pytest.raises(ValueError):
        dec.marker_search(d_bytes, 1000, 0x47, 8, 16, accumulate=True)


# ---- the receivers ------------------------------------------------------------------------------------------------------------

W, HEAD, TAIL, PERIOD = 67, 9, 13, 1024


def marked_stream(seed, phase, frames=8):
    code, pc, dec = decoder()
    bits = mr.frames_with_marker(seed, *CCSDS_ASM, PERIOD, frames, phase)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, np.packbits(bits)[None])
    return bits, synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, 4.0, code.R, np.random.default_rng(seed + 50),
                                      pc.soft_dtype)[0]


def ragged_pushes(rng, T):
    cuts = np.unique(rng.integers(1, T, size=9))
    return [(int(a), int(b)) for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [T]]))]


def whole_stream_search(dec, d_sym):
    out, n_bits = dec.decode_stream(d_sym, begin=True, end=True, window=W, head=HEAD, tail=TAIL)
    d, c, lock = dec.marker_search(out, n_bits, *CCSDS_ASM, PERIOD)
    return out, as_u32(d)[0], as_u32(c)[0], tuple(int(x) for x in as_u32(lock)[0])


def test_stream_decoder_keeps_the_marker_totals():
    import torch
    code, pc, dec = decoder()
    bits, sym = marked_stream(31, 300)
    d_sym = torch.from_numpy(sym).cuda()
    out, want_d, want_c, want_lock = whole_stream_search(dec, d_sym)
    rx = StreamDecoder(dec, W, HEAD, TAIL, marker=CCSDS_ASM, period=PERIOD)
    plain = StreamDecoder(dec, W, HEAD, TAIL)
    assert rx.marker_lock == (0, 0, 0, 0) and not rx.marker_totals[0].any()
    data = b""
    for a, b in ragged_pushes(np.random.default_rng(5), sym.shape[0]):
        data += rx.push(d_sym[a:b])
        plain.push(d_sym[a:b])
    data += rx.finish()
    plain.finish()
    assert data == out.cpu().numpy().tobytes() and rx.calls == plain.calls and len(rx.calls) > 3
    assert any((steps - HEAD - TAIL) % 8 for steps, _, _ in rx.calls[1:-1]), "no call left sub-byte bits to carry"
    got_d, got_c = rx.marker_totals
    assert got_d.dtype == np.int64 and got_d.shape == (PERIOD,)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_c, want_c) and rx.marker_lock == want_lock
    assert want_lock[:2] == (300, 0) and want_c.sum() == bits.size - 31
    with pytest.raises(AttributeError):
        plain.marker_totals


def test_multi_stream_decoder_keeps_the_marker_totals_of_every_stream():
    import torch
    code, pc, dec = decoder()
    phases = (5, 300, 1000)
    syms = [marked_stream(40 + i, ph)[1] for i, ph in enumerate(phases)]
    syms[1] = (pc.soft_decision_high + pc.soft_decision_low - syms[1].astype(np.int64)).astype(syms[1].dtype)       # one stream inverted
    d_sym = torch.from_numpy(np.stack(syms)).cuda()
    wants = [whole_stream_search(dec, d_sym[i]) for i in range(3)]
    rx = MultiStreamDecoder(dec, 3, W, HEAD, TAIL, marker=CCSDS_ASM, period=PERIOD)
    plain = MultiStreamDecoder(dec, 3, W, HEAD, TAIL)
    for a, b in ragged_pushes(np.random.default_rng(6), d_sym.shape[1]):
        rx.push(d_sym[:, a:b])
        plain.push(d_sym[:, a:b])
    rx.finish()
    plain.finish()
    assert rx.calls == plain.calls
    got_d, got_c = rx.marker_totals
    assert got_d.shape == (3, PERIOD)
    for i, (_, want_d, want_c, want_lock) in enumerate(wants):
        assert np.array_equal(got_d[i], want_d) and np.array_equal(got_c[i], want_c) and rx.marker_lock[i] == want_lock, i
        assert want_lock[:2] == (phases[i], int(i == 1))


# ---- end to end: node synchronisation leaves the inversion open, the marker closes it ------------------------------------------

def test_sync_search_then_marker_search_resolves_the_inversion(oracle):
    import torch
    code, pc, dec = decoder()
    high, low = pc.soft_decision_high, pc.soft_decision_low
    Wn, head, tail, P, phase = 64, 48, 48, 256, 77
    T = head + 16 * Wn + tail
    steps = T + 8
    # the emitted bits are those of steps [head, T - tail): the marker stands at phase 77 of THEM
    bits = mr.frames_with_marker(9, *CCSDS_ASM, P, 0, (head + phase) % P, n_bits=steps)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, np.packbits(bits)[None])[:, :steps]
    sym = synth.quantise_numpy(coded, high, low, 4.0, code.R, np.random.default_rng(10), pc.soft_dtype)[0]
    truth = (1, NEG_EVEN | NEG_ODD)
    received = sref.impair(sym.reshape(-1), *truth, high, low, np.random.default_rng(11))
    hyps = enumerate_hypotheses(code.R, "bpsk")
    d_rec = torch.from_numpy(received).cuda()
    err, cmp, best = dec.sync_search(d_rec, hyps, T, window=Wn, head=head, tail=tail)
    err, best = err.cpu().numpy(), int(best.item())
    assert hyps[best] == (1, 0) and err[best] == err[hyps.index(truth)]          # the tie, at the lower index
    stream = dec.sync_build(d_rec, [hyps[best]], T)
    out, n_bits = dec.decode_stream(stream[0], begin=False, end=False, window=Wn, head=head, tail=tail)
    d, c, lock = dec.marker_search(out, n_bits, *CCSDS_ASM, P)
    lock = as_u32(lock)[0]
    assert tuple(lock[:2]) == (phase, 1) and lock[3] == 32 * 4
    upright = sref.build_stream(received, *truth, T, code.R, high, low)
    by, n = sr.stream_reference(oracle, code, oracle_cfg("SOFT16", code.R), upright, Wn, head, tail, flags=0)
    assert n == n_bits
    tx = bits[head:T - tail]
    right = np.unpackbits(by)[:n] == tx
    got = np.unpackbits(~out.cpu().numpy())[:n_bits]
    assert right.mean() > 0.99 and np.array_equal(got[right], tx[right])
