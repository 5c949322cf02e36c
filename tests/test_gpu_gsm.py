"""BatchDecoder.gsm_deinterleave / gsm_fire / gsm_tchfs (vit_hip_gsm_deinterleave_batch, vit_hip_gsm_fire_batch, vit_hip_gsm_tchfs_batch) on
the GPU against the numpy rules of viterbidecodercpp_amd.gsm, on every byte of every output buffer over a fill pattern, written or not:
rows 1 and 3, blocks 1, 2 and 65 (more than one workgroup), both symbol widths, strides with poison between the bursts and rows, every
subset of outputs, the negation at the most negative value, the diagonal history over three calls against one; the Fire code on 256
frames of every kind of damage, in place and out of place, both octet orders; every documented error with a live handle and the outputs
untouched; and the two receivers on the sets of tests/gsm_cases.py, eager and as one captured graph replayed twice, equal to the CPU
chains bit for bit.  No torch.cuda.Stream() call is made here (tests/test_gpu_is95.py says why)."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, GSM_BLOCK, GSM_DIAGONAL, BatchDecoder, GsmControlDecoder, GsmTchfDecoder, _lib, gsm_deinterleave_numpy, gsm_facch_steal_numpy, gsm_fire_numpy,
                                   gsm_tchfs_bursts_numpy, gsm_tchfs_numpy)
from tests import gsm_cases as cases
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

FILL = 0x5A
POISON = -77
NAMES = ("full", "class1", "class2", "steal")


@functools.lru_cache(maxsize=None)
def decoder(decode_type="SOFT16"):
    pc, table, config = make_table_config(cases.CODE, decode_type)
    return pc, BatchDecoder(table, config)


@pytest.fixture(scope="module", autouse=True)
def release_the_decoders():
    yield
    import gc
    import torch
    decoder.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


def filled(shape, dtype, fill=FILL):
    import torch
    n = int(np.prod(shape)) * dtype.itemsize
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


def image(shape, np_dtype, fill=FILL):
    return np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(np_dtype).itemsize), dtype=np_dtype).reshape(shape).copy()


def run_deinterleave(decode_type, rows, m, mode, seed, keep=15, negate=False, pad=(0, 0), hist=None, fill=None, extreme=False):
    """one call: every output buffer (8 guard elements behind it) against the image the numpy rule predicts.  -> the numpy outputs"""
    import torch
    pc, dec = decoder(decode_type)
    rng = np.random.default_rng(seed)
    info = np.iinfo(pc.soft_dtype)
    x = rng.integers(info.min, info.max + 1, size=(rows, 4 * m, 116)).astype(pc.soft_dtype)
    if extreme:
        x[:, ::2] = info.min                                         # -(-128), -(-32768): clamped to the top of the type
    d_in = torch.full((rows, 4 * m + pad[0], 116 + pad[1]), POISON, dtype=dec._soft_dtype, device="cuda")
    d_in[:, :4 * m, :116] = torch.from_numpy(x).cuda()
    want = gsm_deinterleave_numpy(x, mode, negate, hist, fill)
    sizes = {"full": 456, "class1": 378, "class2": 78, "steal": 1}
    bufs = {k: filled((rows * m * sizes[k] + 8,), torch.int32 if k == "steal" else dec._soft_dtype) for k in NAMES}
    bufs["n_out"] = filled((rows + 8,), torch.int32)
    out = {k: bufs[k][:rows * m * sizes[k]] for i, k in enumerate(NAMES) if (keep >> i) & 1}
    out["n_out"] = bufs["n_out"][:rows]
    if mode == GSM_DIAGONAL:
        bufs["hist_out"], bufs["fill_out"] = filled((rows * 464 + 8,), dec._soft_dtype), filled((rows + 8,), torch.int32)
        out["hist_out"], out["fill_out"] = bufs["hist_out"][:rows * 464], bufs["fill_out"][:rows]
    d_hist = None if hist is None else torch.from_numpy(np.ascontiguousarray(hist).reshape(rows, 464)).cuda()
    d_fill = None if fill is None else torch.from_numpy(np.asarray(fill, dtype=np.int32)).cuda()
    view = d_in[:, :4 * m, :116] if rows > 1 or pad != (0, 0) else d_in[0, :, :116]
    got = dec.gsm_deinterleave(view, mode, negate=negate, hist=d_hist, fill=d_fill, out=out)
    torch.cuda.synchronize()
    d_in[:, :4 * m, :116] = POISON
    assert (d_in == POISON).all()
    expect = dict(zip(NAMES + ("n_out", "hist_out", "fill_out"), want))
    for k, buf in bufs.items():
        np_dtype = np.int32 if buf.dtype == torch.int32 else pc.soft_dtype
        e = image(buf.shape, np_dtype)
        if k in out:
            assert got[k].data_ptr() == buf.data_ptr()
            e[:out[k].numel()] = np.asarray(expect[k]).reshape(-1)
        else:
            assert got[k] is None
        assert np.array_equal(buf.cpu().numpy(), e), (decode_type, rows, m, mode, keep, negate, pad, k)
    return want


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("m", [1, 2, 65])
def test_shapes_widths_and_strides(decode_type, rows, m):
    for mode in (GSM_BLOCK, GSM_DIAGONAL):
        run_deinterleave(decode_type, rows, m, mode, 10 * m + rows)
        run_deinterleave(decode_type, rows, m, mode, 20 * m + rows, pad=(4, 7))
        if mode == GSM_DIAGONAL:                                     # with history: some rows have it, some not
            rng = np.random.default_rng(m)
            hist = rng.integers(-100, 100, size=(rows, 4, 116)).astype(decoder(decode_type)[0].soft_dtype)
            run_deinterleave(decode_type, rows, m, mode, 30 * m + rows, pad=(0, 3), hist=hist, fill=[4, 0, 4][:rows])


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_every_subset_of_outputs_and_the_negation(decode_type):
    for keep in range(1, 16):
        run_deinterleave(decode_type, 3, 2, keep % 2, keep, keep=keep, negate=keep % 3 == 0, pad=(0, keep % 2))
    info = np.iinfo(decoder(decode_type)[0].soft_dtype)
    for mode in (GSM_BLOCK, GSM_DIAGONAL):
        hist = np.full((3, 4, 116), info.min, dtype=info.dtype) if mode == GSM_DIAGONAL else None
        want = run_deinterleave(decode_type, 3, 2, mode, 77, negate=True, hist=hist, fill=None if hist is None else [4, 4, 0], extreme=True)
        assert (want[0] == info.max).any() and not (want[0] == info.min).any()       # -128 / -32768 came out as the top of the type
    import torch
    dec = decoder(decode_type)[1]
    got = dec.gsm_deinterleave(torch.zeros((2, 8, 116), dtype=dec._soft_dtype, device="cuda"), "diagonal", want=("class1", "steal"))
    assert {k: None if v is None else tuple(v.shape) for k, v in got.items()} == {
        "hist_out": (2, 464), "fill_out": (2,), "n_out": (2,), "full": None, "class1": (2, 2, 189, 2), "class2": None, "steal": (2, 2)}


def test_diagonal_history_over_three_calls_equals_one_call():
    import torch
    _, dec = decoder()
    x = np.random.default_rng(3).integers(-127, 128, size=(3, 28, 116)).astype(np.int16)
    d = torch.from_numpy(x).cuda()
    whole = dec.gsm_deinterleave(d, GSM_DIAGONAL)
    state = [(torch.zeros((3, 464), dtype=torch.int16, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")) for _ in range(2)]
    parts, turn, hist, fill = [], 0, None, None
    for a, b in ((0, 12), (12, 16), (16, 28)):
        out = {"full": filled((3, (b - a) // 4, 228, 2), torch.int16), "steal": filled((3, (b - a) // 4), torch.int32), "n_out": filled((3,), torch.int32),
               "hist_out": state[turn][0], "fill_out": state[turn][1]}
        got = dec.gsm_deinterleave(d[:, a:b], GSM_DIAGONAL, hist=hist, fill=fill, out=out)
        hist, fill, turn = state[turn][0], state[turn][1], 1 - turn
        torch.cuda.synchronize()
        n = got["n_out"].cpu().numpy()
        assert n.tolist() == [(b - a) // 4 - (a == 0)] * 3
        parts.append((got["full"][:, :n[0]].cpu().numpy(), got["steal"][:, :n[0]].cpu().numpy()))
        assert not got["full"][:, n[0]:].any() and not got["steal"][:, n[0]:].any()
    torch.cuda.synchronize()
    assert whole["n_out"].cpu().numpy().tolist() == [6] * 3
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), whole["full"][:, :6].cpu().numpy())
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), whole["steal"][:, :6].cpu().numpy())
    assert np.array_equal(whole["full"].cpu().numpy(), gsm_deinterleave_numpy(x, GSM_DIAGONAL)[0])


@pytest.mark.parametrize("max_burst", [0, 5, 12])
def test_fire_on_256_frames_in_and_out_of_place(max_burst):
    import torch
    _, dec = decoder()
    frames, _ = cases.fire_frames()
    for lsb in (False, True):
        want_s, want_d = gsm_fire_numpy(frames, max_burst, lsb)
        for stride, in_place in ((28, False), (31, False), (28, True), (31, True)):
            d_in = torch.full((256, stride), 0xEE, dtype=torch.uint8, device="cuda")
            d_in[:, :28] = torch.from_numpy(frames).cuda()
            status = filled((257, 4), torch.int32)
            data = filled((257, 26), torch.uint8)
            out = (status[:256], d_in[:, :28] if in_place else data[:256, :23])
            got_s, got_d = dec.gsm_fire(d_in[:, :28], max_burst, lsb_first=lsb, out=out)
            torch.cuda.synchronize()
            e_s, e_d, e_in = image((257, 4), np.int32), image((257, 26), np.uint8), np.full((256, stride), 0xEE, dtype=np.uint8)
            e_s[:256], e_in[:, :28] = want_s, frames
            (e_in if in_place else e_d[:256])[:, :23] = want_d
            assert np.array_equal(status.cpu().numpy(), e_s), (max_burst, lsb, stride, in_place)
            assert np.array_equal(data.cpu().numpy(), e_d) and np.array_equal(d_in.cpu().numpy(), e_in), (max_burst, lsb, stride, in_place)
    got_s, got_d = dec.gsm_fire(torch.from_numpy(frames[:5]).cuda(), max_burst)
    torch.cuda.synchronize()
    want_s, want_d = gsm_fire_numpy(frames[:5], max_burst)
    assert np.array_equal(got_s.cpu().numpy(), want_s) and np.array_equal(got_d.cpu().numpy(), want_d)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("frames", [1, 3, 261])
def test_tchfs_on_every_byte(decode_type, frames):
    import torch
    pc, dec = decoder(decode_type)
    rng = np.random.default_rng(frames)
    decoded = rng.integers(0, 256, size=(frames, 24), dtype=np.uint8)
    mid = (pc.soft_decision_high + pc.soft_decision_low) // 2
    class2 = rng.integers(mid - 2, mid + 3, size=(frames, 78)).astype(pc.soft_dtype)                       # many at the midpoint
    want_speech, want_status = gsm_tchfs_numpy(decoded, class2, pc.soft_decision_high, pc.soft_decision_low)
    for stride, pad in ((24, 0), (27, 4)):
        d_in = torch.full((frames, stride), 0xEE, dtype=torch.uint8, device="cuda")
        d_in[:, :24] = torch.from_numpy(decoded).cuda()
        speech, status = filled((frames + 1, 33 + pad), torch.uint8), filled((frames + 1, 2), torch.int32)
        dec.gsm_tchfs(d_in[:, :24] if frames > 1 else d_in[0, :24], torch.from_numpy(class2).cuda(), out=(speech[:frames, :33], status[:frames]))
        torch.cuda.synchronize()
        e_speech, e_status = image((frames + 1, 33 + pad), np.uint8), image((frames + 1, 2), np.int32)
        e_speech[:frames, :33], e_status[:frames] = want_speech, want_status
        assert np.array_equal(speech.cpu().numpy(), e_speech) and np.array_equal(status.cpu().numpy(), e_status), (decode_type, frames, stride)
    assert (want_status[:, 1] > 0).any()


def test_rejected_arguments_launch_nothing():
    import torch
    _, dec = decoder()
    lib, h, vp = _lib.load(), dec._handle._h, C.c_void_p
    R, M = 3, 2
    d_in = torch.ones(R * 8 * 120 + 16, dtype=torch.int16, device="cuda")
    hist = [torch.zeros(R * 464 + 8, dtype=torch.int16, device="cuda") for _ in range(2)]
    cnt = [filled((R + 2,), torch.int32) for _ in range(3)]
    outs = [filled((R * M * n + 8,), torch.int16) for n in (456, 378, 78)] + [filled((R * M + 2,), torch.int32)]
    i, hi, ho, fi, fo, no = d_in.data_ptr(), hist[0].data_ptr(), hist[1].data_ptr(), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr()
    o = [x.data_ptr() for x in outs]
    p = lambda a: vp(a) if a else None

    def call(handle=h, at=i, rs=0, bs=0, rows=R, bursts=4 * M, mode=0, flags=0, state=(0, 0, 0, 0), n=no, out=tuple(o)):
        return lib.vit_hip_gsm_deinterleave_batch(handle, p(at), rs, bs, rows, bursts, mode, flags, *[p(a) for a in state], p(n), *[p(a) for a in out], None)

    code3 = next(c for c in COMMON_CODES if c.R != 2)
    _, table3, config3 = make_table_config(code3, "SOFT16")
    bad = [dict(handle=None), dict(at=0), dict(out=(0, 0, 0, 0)), dict(handle=BatchDecoder(table3, config3)._handle._h), dict(mode=2), dict(flags=2),
           dict(state=(hi, fi, 0, 0)), dict(state=(0, 0, ho, fo)), dict(mode=1, state=(hi, 0, 0, 0)), dict(mode=1, state=(0, fi, 0, 0)),
           dict(mode=1, state=(0, 0, ho, 0)), dict(mode=1, state=(0, 0, 0, fo)), dict(bursts=6), dict(bursts=9), dict(at=i + 1), dict(out=(o[0] + 1, 0, 0, 0)),
           dict(out=(0, o[1] + 1, 0, 0)), dict(out=(0, 0, o[2] + 1, 0)), dict(out=(0, 0, 0, o[3] + 2)), dict(n=no + 2), dict(mode=1, state=(hi + 1, fi, 0, 0)),
           dict(mode=1, state=(hi, fi + 2, 0, 0)), dict(mode=1, state=(0, 0, ho + 1, fo)), dict(mode=1, state=(0, 0, ho, fo + 2)), dict(bs=115), dict(rs=8 * 116 - 1),
           dict(rs=(1 << 31) - 1), dict(bs=(1 << 31) - 1), dict(rows=(1 << 31) - 1), dict(bursts=1 << 31), dict(rows=1 << 30, out=(0, 0, 0, o[3])),
           dict(out=(i + 64, 0, 0, 0)), dict(n=i + 64), dict(mode=1, state=(hi, fi, hi, fo)), dict(mode=1, state=(hi, fi, ho, fi)), dict(mode=1, state=(hi, fi, ho, fo), n=fo),
           dict(out=(o[0], o[0] + 64, 0, 0)), dict(out=(0, 0, o[2], o[2] + 64)), dict(mode=1, state=(hi, fi, ho, fo), out=(0, 0, 0, hi + 64))]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(rows=0) == _lib.OK and call(bursts=0) == _lib.OK                           # no work
    torch.cuda.synchronize()
    assert all((x.view(torch.uint8) == FILL).all() for x in outs + cnt) and not hist[1].any()
    assert call(bs=120, mode=1, state=(hi, fi, ho, fo)) == _lib.OK
    torch.cuda.synchronize()
    assert (outs[0][:R * M * 456].view(R, M, 456)[:, 0] == 1).all() and (outs[0][:R * M * 456].view(R, M, 456)[:, 1] == 0).all()      # fill_in was 0x5A5A5A5A: no history
    assert cnt[2][:R].tolist() == [M - 1] * R and cnt[1][:R].tolist() == [4] * R and (hist[1][:R * 464] == 1).all() and not hist[1][R * 464:].any()

    frames = torch.zeros((5, 28), dtype=torch.uint8, device="cuda")
    status, data = filled((5, 4), torch.int32), filled((5, 23), torch.uint8)
    b, s, d = frames.data_ptr(), status.data_ptr(), data.data_ptr()

    def fire(handle=h, at=b, stride=0, n=5, max_burst=12, flags=0, st=s, out=d, ostride=0):
        return lib.vit_hip_gsm_fire_batch(handle, p(at), stride, n, max_burst, flags, p(st), p(out), ostride, None)

    for kw in (dict(handle=None), dict(at=0), dict(st=0), dict(out=0), dict(max_burst=13), dict(flags=2), dict(st=s + 2), dict(stride=27), dict(ostride=22),
               dict(stride=(1 << 31) - 1), dict(ostride=(1 << 31) - 1), dict(n=(1 << 31) - 1), dict(st=b + 8), dict(st=d + 8), dict(out=b), dict(out=b + 1, ostride=28),
               dict(out=b + 28)):
        assert fire(**kw) == _lib.ERR_INVALID_ARG, kw
    assert fire(n=0) == _lib.OK
    torch.cuda.synchronize()
    assert (status.view(torch.uint8) == FILL).all() and (data == FILL).all()
    assert fire(out=b, ostride=28) == _lib.OK                                              # in place
    torch.cuda.synchronize()
    assert np.array_equal(status.cpu().numpy(), gsm_fire_numpy(np.zeros((5, 28), dtype=np.uint8))[0]) and not frames.any()
    assert status[:, 0].tolist() == [-1] * 5                                               # all zeros is no codeword: the parity is 40 ones

    class2 = torch.zeros((5, 78), dtype=torch.int16, device="cuda")
    speech, tstatus = filled((5, 33), torch.uint8), filled((5, 2), torch.int32)
    c, sp, ts = class2.data_ptr(), speech.data_ptr(), tstatus.data_ptr()

    def tchfs(handle=h, at=b, stride=0, c2=c, n=5, out=sp, ostride=0, st=ts):
        return lib.vit_hip_gsm_tchfs_batch(handle, p(at), stride, p(c2), n, p(out), ostride, p(st), None)

    for kw in (dict(handle=None), dict(at=0), dict(c2=0), dict(out=0), dict(c2=c + 1), dict(st=ts + 2), dict(stride=23), dict(ostride=32), dict(stride=(1 << 31) - 1),
               dict(ostride=(1 << 31) - 1), dict(n=(1 << 31) - 1), dict(out=b + 8), dict(out=c + 8), dict(st=b + 8), dict(st=c + 8), dict(st=sp + 8)):
        assert tchfs(**kw) == _lib.ERR_INVALID_ARG, kw
    assert tchfs(n=0) == _lib.OK
    torch.cuda.synchronize()
    assert (speech == FILL).all() and (tstatus.view(torch.uint8) == FILL).all()
    assert tchfs(st=0) == _lib.OK                                                          # the status is optional
    torch.cuda.synchronize()
    assert not speech.any() and (tstatus.view(torch.uint8) == FILL).all()

    # the Python layer
    sym = d_in[:R * 8 * 116].view(R, 8, 116)
    for bad_call in (lambda: dec.gsm_deinterleave(sym[:, :6], 0), lambda: dec.gsm_deinterleave(sym, 2), lambda: dec.gsm_deinterleave(sym, 0, hist=hist[0][:R * 464], fill=cnt[0][:R]),
                     lambda: dec.gsm_deinterleave(sym, 1, hist=hist[0][:R * 464]), lambda: dec.gsm_deinterleave(sym, 0, out={"n_out": cnt[2][:R]}),
                     lambda: dec.gsm_deinterleave(sym, 0, out={"full": outs[0][:R * M * 456 - 1]}), lambda: dec.gsm_deinterleave(sym, 0, out={"full": outs[0][:R * M * 456], "more": 1}),
                     lambda: dec.gsm_deinterleave(sym, 0, out={"full": outs[0][:R * M * 456], "hist_out": hist[1][:R * 464], "fill_out": cnt[1][:R]}),
                     lambda: dec.gsm_deinterleave(sym.view(torch.int8)[:, :, :116], 0), lambda: BatchDecoder(table3, config3).gsm_deinterleave(sym, 0),
                     lambda: dec.gsm_fire(frames, 13), lambda: dec.gsm_fire(frames[:, :27]), lambda: dec.gsm_fire(frames, out=(status, data[:4])),
                     lambda: dec.gsm_tchfs(frames[:, :23], class2), lambda: dec.gsm_tchfs(frames, class2[:4]), lambda: GsmControlDecoder(BatchDecoder(table3, config3))):
        with pytest.raises(ValueError):
            bad_call()


def test_the_control_receiver_eager_and_as_a_graph_replayed_twice():
    import torch
    _, dec = decoder()
    assert dec.plan == _lib.PLAN_REG and "GENERIC" in dec.plan_note, dec.plan_note
    bursts, l2, (want_l2, want_status) = cases.control_set()
    assert np.array_equal(want_l2, l2)                                                     # the condition tests/test_gsm_cpu.py holds
    rx = GsmControlDecoder(dec)
    got_l2, got_status = rx.push(torch.from_numpy(bursts).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got_l2.cpu().numpy(), want_l2) and np.array_equal(got_status.cpu().numpy(), want_status)
    # two rows of four blocks, the octets LSB-first
    two = np.ascontiguousarray(bursts.reshape(2, 16, 116))
    got = GsmControlDecoder(dec, lsb_first=True).push(torch.from_numpy(two).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), cases.control_chain(bursts, lsb_first=True)[0])
    # the negated stream with the flag
    got = GsmControlDecoder(dec, negate=True).push(torch.from_numpy(-bursts).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want_l2)
    d_in = torch.zeros((1, 32, 116), dtype=torch.int16, device="cuda")
    out = (torch.zeros((8, 23), dtype=torch.uint8, device="cuda"), torch.zeros((8, 4), dtype=torch.int32, device="cuda"))
    rx.push(d_in, out=out)                                                                 # the buffers and the workspace stand before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rx.push(d_in, out=out)
    second = np.ascontiguousarray(bursts[:, ::-1])                                         # other input: the bursts in reverse order
    for replay, x in enumerate((bursts, second)):
        d_in.copy_(torch.from_numpy(x).cuda())
        graph.replay()
        torch.cuda.synchronize()
        w_l2, w_status = cases.control_chain(x)
        assert np.array_equal(out[0].cpu().numpy(), w_l2) and np.array_equal(out[1].cpu().numpy(), w_status), replay
    assert not np.array_equal(cases.control_chain(second)[0], want_l2)


def check_traffic(got, want, label):
    """the five outputs of a push over the slots the host chain filled"""
    n = int(want[5][0])
    for k in range(5):
        assert np.array_equal(got[k].cpu().numpy()[:n], want[k][:n]), (label, k)
    return n


def test_the_traffic_receiver_eager_and_as_a_graph_replayed_twice():
    import torch
    _, dec = decoder()
    bursts, speech, l2 = cases.traffic_set()
    pushes = [bursts[None, :12], bursts[None, 12:24], bursts[None, 24:36]]
    want = cases.traffic_chain(pushes)
    rx = GsmTchfDecoder(dec)
    got_speech, got_facch, got_steal = [], [], []
    for i, x in enumerate(pushes):
        got = rx.push(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        torch.cuda.synchronize()
        n = check_traffic(got, want[i], i)
        assert rx.n_out.cpu().numpy().tolist() == [n] == [3 - (i == 0)]
        got_speech.append(got[0].cpu().numpy()[:n]), got_facch.append(got[2].cpu().numpy()[:n]), got_steal.append(got[4].cpu().numpy()[:n])
    keep = np.arange(8) != cases.STOLEN
    assert np.array_equal(np.concatenate(got_speech)[keep], speech[keep]) and np.array_equal(np.concatenate(got_facch)[cases.STOLEN], l2)
    assert (np.concatenate(got_steal) > 0).tolist() == (~keep).tolist()
    # one graph of TWO pushes (the history goes there and back), replayed twice: four pushes of one sequence, the first without history
    rx = GsmTchfDecoder(dec)
    rng = np.random.default_rng(cases.SEED + 2)
    seq = gsm_facch_steal_numpy(gsm_tchfs_bursts_numpy(np.concatenate([speech, speech[:3]])), 5, l2)       # 11 blocks, 48 bursts: four pushes of 12
    seq = cases.flip(seq, 11, GSM_DIAGONAL, rng, 378)
    pushes = [np.ascontiguousarray(seq[None, 12 * i:12 * i + 12]) for i in range(4)]
    want = cases.traffic_chain(pushes)
    d_in = [torch.zeros((1, 12, 116), dtype=torch.int16, device="cuda") for _ in range(2)]
    outs = [(torch.zeros((3, 33), dtype=torch.uint8, device="cuda"), torch.zeros((3, 2), dtype=torch.int32, device="cuda"), torch.zeros((3, 23), dtype=torch.uint8, device="cuda"),
             torch.zeros((3, 4), dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")) for _ in range(2)]
    rx.push(d_in[0], out=outs[0]), rx.push(d_in[1], out=outs[1])                           # the buffers and workspaces stand before the capture
    rx.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rx.push(d_in[0], out=outs[0]), rx.push(d_in[1], out=outs[1])
    for replay in range(2):
        for k in range(2):
            d_in[k].copy_(torch.from_numpy(pushes[2 * replay + k]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        for k in range(2):
            assert check_traffic(outs[k], want[2 * replay + k], (replay, k)) == 3 - (replay == 0 and k == 0)
