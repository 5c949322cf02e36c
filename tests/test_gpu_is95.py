"""BatchDecoder.is95_deinterleave / is95_rate_decide (vit_hip_is95_deinterleave_batch, vit_hip_is95_rate_decide_batch) on the GPU against
the numpy rules of viterbidecodercpp_amd.is95, on every byte of every output buffer from two different fills, written or not: frame
counts on both sides of the frames-per-workgroup boundary, both symbol widths, no mask / one / per frame, input strides with poison
between the frames, every subset of outputs, shifts and clamps with the inputs at both extremes of the type, the decision with poisoned
count memory and absent hypotheses; the error counts of the four hypotheses in one call against four channel_errors calls; every
documented error with a live handle and the outputs untouched; and Is95TrafficDecoder on the
noisy set of tests/is95_cases.py at both polynomial sets, eager and as one captured graph replayed on new input twice, equal to the CPU
chain bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, IS95_RATE_SET_1, BatchDecoder, Is95TrafficDecoder, _lib, is95_deinterleave_numpy,
                                   is95_rate_decide_numpy)
from tests import is95_cases as cases
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

FILLS = (0x5A, 0xC3)
FRAME_COUNTS = (1, 3, 4, 5, 65, 257)
POISON = -77


@functools.lru_cache(maxsize=None)
def decoder(decode_type="SOFT16", name="stock"):
    pc, table, config = make_table_config(cases.CODES[name], decode_type)
    return pc, BatchDecoder(table, config)


@pytest.fixture(scope="module", autouse=True)
def release_the_decoders():
    """the cached decoders go when this module is done: a handle owns a stream.  No test here calls torch.cuda.Stream(): every such call
    takes the next of torch's pool of 32 streams, round robin, each bound for good to one of the process's four hardware queues when it
    was first used, so a module that makes such calls moves every later test of the process along that pool.
    tests/test_gpu_residency.py needs its two consecutive pool streams on different hardware queues, and with two calls from this
    module in front of it its CDMA 2000 case drew a pair on one queue: the chainback then waits behind the spinning waves whatever the
    registers allow.  The graphs below are captured on the stream torch.cuda.graph keeps for that, which the modules in front of this
    one have long made"""
    yield
    import gc
    import torch
    decoder.cache_clear()
    gc.collect()
    torch.cuda.synchronize()


def filled(shape, dtype, fill):
    import torch
    n = int(np.prod(shape)) * dtype.itemsize
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda").view(dtype).view(*shape)


def image(shape, np_dtype, fill):
    return np.frombuffer(bytes([fill]) * (int(np.prod(shape)) * np.dtype(np_dtype).itemsize), dtype=np_dtype).reshape(shape).copy()


def run_deinterleave(decode_type, frames, seed, mask_kind, pad, keep, shift, clamp, extreme=None):
    """one call from both fills: every output buffer (8 guard elements behind it) against the image the numpy rule predicts"""
    import torch
    pc, dec = decoder(decode_type)
    rng = np.random.default_rng(seed)
    info = np.iinfo(pc.soft_dtype)
    x = rng.integers(info.min, info.max + 1, size=(frames, 384)).astype(pc.soft_dtype)
    if extreme is not None:
        x[:] = info.min if extreme < 0 else info.max
    d_in = torch.full((frames, 384 + pad), POISON, dtype=dec._soft_dtype, device="cuda")
    d_in[:, :384] = torch.from_numpy(x).cuda()
    masks = rng.integers(0, 256, size=(frames, 48 + 3), dtype=np.uint8)
    if extreme is not None:
        masks[::2] = 0xFF                                              # every other frame wholly negated: -min adds as +min's magnitude
    scramble = [None, masks[0, :48].copy(), masks[:, :48]][mask_kind]
    d_mask = [None, torch.from_numpy(masks[0, :48].copy()).cuda(), torch.from_numpy(masks).cuda()[:, :48]][mask_kind]      # rows 51 bytes apart
    lo, hi = (pc.soft_decision_low, pc.soft_decision_high) if clamp is None else clamp
    want = is95_deinterleave_numpy(x, scramble, shift, lo, hi)
    for fill in FILLS:
        bufs = [filled((frames * (384 >> h) + 8,), dec._soft_dtype, fill) for h in range(4)]
        out = tuple(bufs[h][:frames * (384 >> h)].view(frames, 192 >> h, 2) if (keep >> h) & 1 else None for h in range(4))
        got = dec.is95_deinterleave(d_in[:, :384] if frames > 1 or pad == 0 else d_in[0, :384], scramble=d_mask, shift=shift, clamp=clamp, out=out)
        torch.cuda.synchronize()
        assert (d_in[:, 384:] == POISON).all()
        for h in range(4):
            expect = image((frames * (384 >> h) + 8,), pc.soft_dtype, fill)
            if (keep >> h) & 1:
                assert got[h].data_ptr() == bufs[h].data_ptr()
                expect[:frames * (384 >> h)] = want[h].reshape(-1)
            else:
                assert got[h] is None
            assert np.array_equal(bufs[h].cpu().numpy(), expect), (decode_type, frames, mask_kind, pad, keep, shift, clamp, h, fill)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("frames", FRAME_COUNTS)
def test_frame_counts_masks_and_strides(decode_type, frames):
    for mask_kind in range(3):
        run_deinterleave(decode_type, frames, 10 * frames + mask_kind, mask_kind, pad=(0, 1, 9)[mask_kind], keep=15, shift=0, clamp=None)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
def test_every_subset_of_outputs(decode_type):
    for keep in range(1, 16):
        run_deinterleave(decode_type, 5, keep, keep % 3, pad=2 * (keep % 2), keep=keep, shift=keep % 4, clamp=None)
    import torch
    dec = decoder(decode_type)[1]
    out = dec.is95_deinterleave(torch.zeros((2, 384), dtype=dec._soft_dtype, device="cuda"), want=(True, False, False, True))
    assert [None if o is None else tuple(o.shape) for o in out] == [(2, 192, 2), None, None, (2, 24, 2)]


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
def test_shifts_and_clamps_with_inputs_at_both_extremes(decode_type):
    """HARD8 is the width at which the decoder's own clamp (-1, 1) saturates every sum of two and more"""
    info = np.iinfo(decoder(decode_type)[0].soft_dtype)
    full = (int(info.min), int(info.max))
    for extreme in (-1, 1):
        for shift in (0, 3):
            run_deinterleave(decode_type, 5, 3, 2, pad=4, keep=15, shift=shift, clamp=full, extreme=extreme)       # the int32 sum of eight
            run_deinterleave(decode_type, 5, 4, 2, pad=0, keep=15, shift=shift, clamp=None, extreme=extreme)       # ... under the decoder's clamp
    for clamp in ((-5, 90) if decode_type == "SOFT16" else (-2, 1), (7, 7), (full[0], full[0])):                   # narrower than the type
        run_deinterleave(decode_type, 9, 5, 1, pad=1, keep=15, shift=1, clamp=clamp)
    run_deinterleave(decode_type, 9, 6, 2, pad=0, keep=15, shift=15, clamp=full)
    if decode_type == "HARD8":                                                                                      # hard decisions in, +-1
        import torch
        pc, dec = decoder(decode_type)
        assert (pc.soft_decision_low, pc.soft_decision_high) == (-1, 1)
        rng = np.random.default_rng(8)
        x = (2 * rng.integers(0, 2, size=(7, 384)) - 1).astype(np.int8)
        mask = rng.integers(0, 256, size=(7, 48), dtype=np.uint8)
        got = dec.is95_deinterleave(torch.from_numpy(x).cuda(), scramble=torch.from_numpy(mask).cuda())
        want = is95_deinterleave_numpy(x, mask, 0, -1, 1)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
        assert set(np.unique(want[0]).tolist()) == {-1, 1} and set(np.unique(want[3]).tolist()) == {-1, 0, 1}


def decide_inputs(frames, seed, present, small):
    rng = np.random.default_rng(seed)
    hi = 6 if small else 1 << 32
    decoded = [rng.integers(0, 256, size=(frames, r.n_bytes + h), dtype=np.uint8) for h, r in enumerate(IS95_RATE_SET_1)]      # rows wider by h
    errors = [rng.integers(0, hi, size=frames, dtype=np.int64) for _ in range(4)]
    compared = [rng.integers(0, 2 * hi, size=frames, dtype=np.int64) % (1 << 32) for _ in range(4)]
    syndrome = [np.where(rng.integers(0, 3, size=frames) != 0, 0, rng.integers(1, 1 << 32, size=frames, dtype=np.int64)) for _ in range(2)]
    return [d if p else None for d, p in zip(decoded, present)], errors, compared, syndrome


@pytest.mark.parametrize("frames", [1, 255, 257])
def test_the_decision_on_every_byte(frames):
    import torch
    _, dec = decoder()
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()
    for case, present in enumerate([(True,) * 4, (False, True, True, True), (False, False, True, False), (True, False, False, True), (True, False, False, False)]):
        small = case % 2 == 0
        decoded, errors, compared, syndrome = decide_inputs(frames, 100 * frames + case, present, small)
        num, den = ((1, 2, 1, 3), 4) if small else ((0xFFFFFFFF, 1 << 31, 3, 1 << 30), 0xFFFFFFFF)
        want_d, want_i = is95_rate_decide_numpy([None if d is None else d[:, :IS95_RATE_SET_1[h].n_bytes] for h, d in enumerate(decoded)], errors,
                                                compared, syndrome, num, den)
        d_bytes = [None if d is None else torch.from_numpy(d).cuda()[:, :IS95_RATE_SET_1[h].n_bytes] for h, d in enumerate(decoded)]
        # the counts of a present hypothesis hold whatever the generator gave, wild values included; those of an absent one are bait:
        # no error, one symbol compared, a zero syndrome would win every frame if they were read
        d_err = [dev(e) if p else dev(np.zeros(frames)) for e, p in zip(errors, present)]
        d_cmp = [dev(c) if p else dev(np.ones(frames)) for c, p in zip(compared, present)]
        d_syn = [dev(s) if p else dev(np.zeros(frames)) for s, p in zip(syndrome, present)]
        for fill in FILLS:
            decision = filled((frames + 1, 4), torch.int32, fill)
            info = filled((frames + 1, 22 + 3), torch.uint8, fill)
            got_d, got_i = dec.is95_rate_decide(d_bytes, d_err, d_cmp, d_syn, num, den, out=(decision[:frames], info[:frames, :22]))
            torch.cuda.synchronize()
            expect_d = image((frames + 1, 4), np.uint32, fill)
            expect_d[:frames] = want_d
            expect_i = image((frames + 1, 25), np.uint8, fill)
            expect_i[:frames, :22] = want_i
            assert np.array_equal(decision.cpu().numpy().view(np.uint32), expect_d), (frames, present, fill)
            assert np.array_equal(info.cpu().numpy(), expect_i), (frames, present, fill)
        got_d, got_i = dec.is95_rate_decide(d_bytes, d_err, d_cmp, d_syn, num, den)
        torch.cuda.synchronize()
        assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want_d) and np.array_equal(got_i.cpu().numpy(), want_i)


def test_rejected_arguments_launch_nothing():
    import torch
    pc, dec = decoder()
    _, dec8 = decoder("SOFT8")
    lib, h = _lib.load(), dec._handle._h
    F = 5
    d_in = torch.ones(F * 400, dtype=torch.int16, device="cuda")
    mask = torch.zeros(F * 48 + 16, dtype=torch.uint8, device="cuda")
    outs = [filled((F * (384 >> k) + 8,), torch.int16, 0x5A) for k in range(4)]
    i, m, o = d_in.data_ptr(), mask.data_ptr(), [x.data_ptr() for x in outs]
    vp = C.c_void_p

    def call(handle=h, at_in=i, stride=0, frames=F, at_mask=m, mstride=0, shift=0, lo=-127, hi=127, out=tuple(o), array=True):
        four = (vp * 4)(*[vp(a) if a else None for a in out]) if array else None
        return lib.vit_hip_is95_deinterleave_batch(handle, vp(at_in) if at_in else None, stride, frames, vp(at_mask) if at_mask else None, mstride,
                                                   shift, lo, hi, four, None)

    bad = [dict(handle=None), dict(at_in=0), dict(array=False), dict(out=(0, 0, 0, 0)), dict(shift=16), dict(lo=1, hi=0), dict(lo=-32769), dict(hi=32768),
           dict(at_in=i + 1), dict(out=(o[0] + 2, o[1], o[2], o[3])), dict(out=(0, 0, 0, o[3] + 1)), dict(stride=383), dict(mstride=47),
           dict(stride=(1 << 31) - 1), dict(mstride=(1 << 31) - 1), dict(frames=(1 << 31) - 1), dict(out=(i + 8, 0, 0, 0)), dict(out=(0, m + 4, 0, 0)),
           dict(out=(0, m + 48, 0, 0), mstride=48), dict(out=(o[0], o[0] + 64, 0, 0)), dict(out=(o[3] + 4, 0, 0, o[3]))]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(handle=dec8._handle._h, lo=-129) == _lib.ERR_INVALID_ARG and call(handle=dec8._handle._h, hi=128) == _lib.ERR_INVALID_ARG
    code3 = next(c for c in COMMON_CODES if c.R != 2)
    _, table3, config3 = make_table_config(code3, "SOFT16")
    assert call(handle=BatchDecoder(table3, config3)._handle._h) == _lib.ERR_INVALID_ARG and b"1/2" in lib.vit_hip_last_error()
    assert call(frames=0) == _lib.OK                                                       # no work
    torch.cuda.synchronize()
    assert all((x.view(torch.uint8) == 0x5A).all() for x in outs)
    assert call(stride=400, mstride=48) == _lib.OK
    torch.cuda.synchronize()
    for k, x in enumerate(outs):
        assert (x[:F * (384 >> k)] == min(1 << k, 127)).all() and (x[F * (384 >> k):].view(torch.uint8) == 0x5A).all()

    decoded = [torch.zeros((F, r.n_bytes), dtype=torch.uint8, device="cuda") for r in IS95_RATE_SET_1]
    cnt = [torch.ones(F + 2, dtype=torch.int32, device="cuda") for _ in range(10)]
    decision = filled((F, 4), torch.int32, 0x5A)
    info = filled((F, 22), torch.uint8, 0x5A)
    b, c, dd, ii = [x.data_ptr() for x in decoded], [x.data_ptr() for x in cnt], decision.data_ptr(), info.data_ptr()

    def decide(handle=h, by=tuple(b), st=(0, 0, 0, 0), er=tuple(c[:4]), cm=tuple(c[4:8]), sy=tuple(c[8:]), frames=F, num=(1, 1, 1, 1), den=10,
               at_dec=dd, at_info=ii, istride=0, arrays=(True,) * 6):
        arr = lambda xs, n: (vp * n)(*[vp(a) if a else None for a in xs])
        args = [arr(by, 4), (C.c_size_t * 4)(*st), arr(er, 4), arr(cm, 4), arr(sy, 2), (C.c_uint32 * 4)(*num)]
        args = [a if keep else None for a, keep in zip(args, arrays)]
        return lib.vit_hip_is95_rate_decide_batch(handle, args[0], args[1], args[2], args[3], args[4], frames, args[5], den, vp(at_dec) if at_dec else None,
                                                  vp(at_info) if at_info else None, istride, None)

    bad = [dict(handle=None), dict(at_dec=0), dict(at_info=0), dict(by=(0, 0, 0, 0)), dict(den=0), dict(er=(0,) + tuple(c[1:4])), dict(cm=(c[4], c[5], 0, c[7])),
           dict(sy=(c[8], 0)), dict(st=(22, 0, 0, 0)), dict(st=(0, 0, 0, 1)), dict(st=(0, 0, (1 << 31) - 1, 0)), dict(istride=21), dict(istride=(1 << 31) - 1),
           dict(at_dec=dd + 2), dict(er=(c[0] + 2,) + tuple(c[1:4])), dict(frames=(1 << 31) - 1), dict(at_info=dd + 40), dict(at_info=b[0] + 8),
           dict(at_dec=c[5] + 4), dict(at_dec=c[9] + 4)]
    bad += [dict(arrays=tuple(k != j for k in range(6))) for j in (0, 2, 3, 4, 5)]
    for kw in bad:
        assert decide(**kw) == _lib.ERR_INVALID_ARG, kw
    assert decide(frames=0) == _lib.OK
    torch.cuda.synchronize()
    assert (decision.view(torch.uint8) == 0x5A).all() and (info == 0x5A).all()
    assert decide(arrays=(True, False, True, True, True, True)) == _lib.OK                 # no stride array: 23, 11, 5, 2
    assert decide(by=(0, b[1], 0, 0), er=(0, c[1], 0, 0), cm=(0, c[5], 0, 0), sy=(0, c[9])) == _lib.OK
    torch.cuda.synchronize()
    assert decision.cpu().numpy().tolist() == [[4, 0, 0, 0]] * F and (info == 0).all()     # errors = compared = 1: above 1 / 10

    # the Python layer: outputs that share storage, wrong shapes, wrong decoders
    sym = d_in[:F * 384].view(F, 384)
    whole = torch.zeros(F * 384 + 64, dtype=torch.int16, device="cuda")
    for out in ((whole[:F * 384], whole[:F * 192], None, None), (whole[:F * 384], None, None, whole[F * 384 - 2:F * 384 - 2 + F * 48]), (None,) * 4,
                (whole[:F * 384],) * 3, (whole[:F * 384 - 1], None, None, None), (whole[:F * 384].view(torch.int8)[:F * 384], None, None, None)):
        with pytest.raises(ValueError):
            dec.is95_deinterleave(sym, out=out)
    for kw in (dict(shift=16), dict(clamp=(1, 0)), dict(scramble=mask[:47]), dict(scramble=mask[:4 * 48].view(4, 48))):
        with pytest.raises(ValueError):
            dec.is95_deinterleave(sym, **kw)
    with pytest.raises(ValueError):
        dec.is95_deinterleave(d_in[:F * 383].view(F, 383))
    with pytest.raises(ValueError):
        BatchDecoder(table3, config3).is95_deinterleave(sym)
    with pytest.raises(ValueError):
        Is95TrafficDecoder(decoder("SOFT16", "stock")[1], max_ser=((1, 1, 1), 10))
    torch.cuda.synchronize()
    assert (whole == 0).all()


@pytest.mark.parametrize("name", ["stock", "standard"])
def test_the_error_counts_in_one_call_equal_channel_errors(name):
    """is95_channel_errors against four channel_errors calls on the noisy set's decodes, from both fills; a subset; strides; and twice in a
    row: the counters are overwritten, not added to"""
    import torch
    _, dec = decoder("SOFT16", name)
    symbols, scramble, rates, info, _ = cases.noisy_set(name)
    F = symbols.shape[0]
    sym = dec.is95_deinterleave(torch.from_numpy(symbols).cuda(), scramble=torch.from_numpy(scramble).cuda())
    wide = [torch.full((F, r.n_bytes + h), 0xEE, dtype=torch.uint8, device="cuda") for h, r in enumerate(IS95_RATE_SET_1)]
    decoded = [w[:, :r.n_bytes] for w, r in zip(wide, IS95_RATE_SET_1)]                     # rows wider by h
    for h, r in enumerate(IS95_RATE_SET_1):
        decoded[h].copy_(dec.decode(sym[h], r.L))
    want = [dec.channel_errors(sym[h], decoded[h], r.L) for h, r in enumerate(IS95_RATE_SET_1)]
    torch.cuda.synchronize()
    assert all((w[0] > 0).any() and (w[1] > 0).all() for w in want)
    for present in ((True,) * 4, (True, False, False, True), (False, False, True, False)):
        for fill in FILLS:
            bufs = [filled((2, F + 1), torch.int32, fill) for _ in range(4)]
            args = ([s if p else None for s, p in zip(sym, present)], [d if p else None for d, p in zip(decoded, present)])
            for _ in range(2):
                errors, compared = dec.is95_channel_errors(*args, out=([b[0, :F] for b in bufs], [b[1, :F] for b in bufs]))
            torch.cuda.synchronize()
            for h in range(4):
                expect = image((2, F + 1), np.int32, fill)
                if present[h]:
                    expect[0, :F], expect[1, :F] = want[h][0].cpu().numpy(), want[h][1].cpu().numpy()
                assert np.array_equal(bufs[h].cpu().numpy(), expect), (present, fill, h)
    errors, compared = dec.is95_channel_errors(sym, decoded)
    torch.cuda.synchronize()
    assert all(torch.equal(errors[h], want[h][0]) and torch.equal(compared[h], want[h][1]) for h in range(4))
    # rejected: nothing launched, the counters as they were
    lib, vp = _lib.load(), C.c_void_p
    cnt = [filled((F,), torch.int32, 0x5A) for _ in range(8)]
    arr = lambda xs: (vp * 4)(*[vp(x) if x else None for x in xs])
    s_, b_, e_, c_ = [x.data_ptr() for x in sym], [x.data_ptr() for x in decoded], [x.data_ptr() for x in cnt[:4]], [x.data_ptr() for x in cnt[4:]]

    def call(handle=dec._handle._h, s=s_, b=b_, st=(0, 12, 7, 5), frames=F, e=e_, c=c_):
        return lib.vit_hip_is95_channel_errors_batch(handle, arr(s) if s else None, arr(b) if b else None, (C.c_size_t * 4)(*st), frames,
                                                     arr(e) if e else None, arr(c) if c else None, None)

    k7 = BatchDecoder(*make_table_config(COMMON_CODES[2], "SOFT16")[1:])
    for kw in (dict(handle=None), dict(handle=k7._handle._h), dict(s=None), dict(b=None), dict(e=None), dict(c=None), dict(b=[0, 0, 0, 0]), dict(s=[0] + s_[1:]),
               dict(e=[0] + e_[1:]), dict(c=c_[:3] + [0]), dict(s=[s_[0] + 1] + s_[1:]), dict(e=[e_[0] + 2] + e_[1:]), dict(st=(22, 12, 7, 5)), dict(st=(0, 0, 0, 1)),
               dict(frames=(1 << 31) - 1), dict(e=[e_[0], e_[0], e_[2], e_[3]]), dict(c=[e_[1] + 4] + c_[1:]), dict(c=[b_[0] + 4] + c_[1:]), dict(e=[s_[3] + 8] + e_[1:])):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(frames=0) == _lib.OK
    torch.cuda.synchronize()
    assert all((x.view(torch.uint8) == 0x5A).all() for x in cnt)
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert all(torch.equal(cnt[h], want[h][0]) and torch.equal(cnt[4 + h], want[h][1]) for h in range(4))
    # a two-valued table that is no convolutional code's: nothing to encode with, nothing launched
    pc, table, config = make_table_config(cases.CODES[name], "SOFT16")
    table._table[0, 5] = pc.soft_decision_high + pc.soft_decision_low - table._table[0, 5]
    odd = BatchDecoder(table, config)
    assert odd._handle.info.table_is_linear == 0
    for x in cnt:
        x.view(torch.uint8).fill_(0x5A)
    assert call(handle=odd._handle._h) == _lib.ERR_UNSUPPORTED and call(handle=odd._handle._h, frames=0) == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.VitHipError):
        odd.is95_channel_errors(sym, decoded)
    torch.cuda.synchronize()
    assert all((x.view(torch.uint8) == 0x5A).all() for x in cnt)
    for bad in (lambda: dec.is95_channel_errors(sym[:3], decoded), lambda: dec.is95_channel_errors([None] + list(sym[1:]), decoded),
                lambda: dec.is95_channel_errors(sym, [None] * 4), lambda: dec.is95_channel_errors(sym, decoded, out=([cnt[0]] * 4, cnt[4:])),
                lambda: k7.is95_channel_errors(sym, decoded)):
        with pytest.raises(ValueError):
            bad()


def push_equals_cpu(name, rx, symbols, scramble, want):
    import torch
    decision, info = rx.push(torch.from_numpy(symbols).cuda(), torch.from_numpy(scramble).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(decision.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(info.cpu().numpy(), want[1]), name


@pytest.mark.parametrize("name", ["stock", "standard"])
def test_the_traffic_decoder_on_the_noisy_set(name):
    """64 frames of mixed rates at the recorded seed and SNR: decisions and info bytes equal to the CPU chain, bit for bit, and with it to
    what was sent"""
    _, dec = decoder("SOFT16", name)
    if name == "standard":
        assert dec.plan == _lib.PLAN_REG and "GENERIC" in dec.plan_note, dec.plan_note
    symbols, scramble, rates, info, (want_d, want_i, _, _) = cases.noisy_set(name)
    assert want_d[:, 0].tolist() == rates.tolist() and np.array_equal(want_i, info)        # the condition tests/test_is95_cpu.py holds
    rx = Is95TrafficDecoder(dec, max_ser=cases.MAX_SER)
    push_equals_cpu(name, rx, symbols, scramble, (want_d, want_i))
    # a threshold nothing meets erases every frame
    import torch
    decision, got = Is95TrafficDecoder(dec, max_ser=((0, 0, 0, 0), 1)).push(torch.from_numpy(symbols).cuda(), torch.from_numpy(scramble).cuda())
    torch.cuda.synchronize()
    zero = want_d[:, 2] == 0
    assert (decision[:, 0].cpu().numpy()[~zero] == 4).all() and (got.cpu().numpy()[~zero] == 0).all()


@pytest.mark.parametrize("name", ["stock", "standard"])
def test_the_whole_push_as_one_graph_replayed_on_new_input_twice(name):
    """one graph of 64 frames, replayed on the recorded noisy set and then on a second set (seed 41, 1 dB above it): each replay returns
    what was sent, equal to the CPU chain bit for bit"""
    import torch
    _, dec = decoder("SOFT16", name)
    code = cases.CODES[name]
    rx = Is95TrafficDecoder(dec, max_ser=cases.MAX_SER)
    F = cases.NOISY_FRAMES
    d_sym = torch.zeros((F, 384), dtype=torch.int16, device="cuda")
    d_mask = torch.zeros((F, 48), dtype=torch.uint8, device="cuda")
    out = (torch.zeros((F, 4), dtype=torch.int32, device="cuda"), torch.zeros((F, 22), dtype=torch.uint8, device="cuda"))
    rx.push(d_sym, d_mask, out=out)                                                        # the buffers and workspaces stand before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rx.push(d_sym, d_mask, out=out)
    symbols, scramble, rates, info, (want_d, want_i, _, _) = cases.noisy_set(name)
    second = cases.make_frames(code, seed=41, snr_db=cases.NOISY_SNR_DB + 1.0)
    sets = [(symbols, scramble, rates, info, want_d, want_i), second + tuple(cases.cpu_chain(code, second[0], second[1])[:2])]
    for replay, (symbols, scramble, rates, info, want_d, want_i) in enumerate(sets):
        d_sym.copy_(torch.from_numpy(symbols).cuda())
        d_mask.copy_(torch.from_numpy(scramble).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want_d) and np.array_equal(out[1].cpu().numpy(), want_i), replay
        assert want_d[:, 0].tolist() == rates.tolist() and np.array_equal(want_i, info), replay
    assert not np.array_equal(sets[0][4], sets[1][4])
