"""LTE rate de-matching on the GPU: vit_hip_lte_rate_dematch_batch / BatchDecoder.lte_rate_dematch against the scalar loop of
tests/lte_reference.py.  D {1, 7, 31, 32, 33, 40, 43, 64, 65, 70, 341, 1024} x E {1, 3D-1, 3D, 3D+1, 2*3D+5, 72, 144, 288, 576, 1920, 16*3D}
(punctured, an exact fit, a ragged last wrap, many wraps) on SOFT16, SOFT8 and HARD8 handles with full-scale inputs, shift {0, 1, 4} with
sums at the rounding boundary and negative, 1, 3 and 300 frames; the whole output compared over a poison fill with a guard behind it, the
input compared afterwards; strides, odd and overlapping offsets, counts of 0, a part, E_max and above, offsets at and past the end of the
input (which ends its allocation); no mask, a region's, a shared one; every rejection; the call in a graph, and with decode_tail_biting
and crc_check in one; the PDCCH and PBCH routes end to end."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, LTE_CRC16, BatchDecoder, _lib, crc_append_numpy, crc_field_numpy, crc_numpy,
                                   lte_gold_sequence, lte_rate_dematch_numpy, lte_rate_match_numpy, pdcch_candidates, synth)
from tests import lte_reference as ref
from tests.helpers import make_table_config, oracle_cfg
from tests.tb_reference import tb_reference

pytestmark = pytest.mark.gpu

DS = (1, 7, 31, 32, 33, 40, 43, 64, 65, 70, 341, 1024)


def es(D):
    n3 = 3 * D
    return sorted({1, n3 - 1, n3, n3 + 1, 2 * n3 + 5, 72, 144, 288, 576, 1920, 16 * n3})


@functools.lru_cache(maxsize=None)
def decoder(decode_type="SOFT16"):
    code = COMMON_CODES[3]
    assert (code.K, code.R) == (7, 3)
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config)


def limits(dtype):
    return (-32768, 32767, ref.POISON16) if dtype == np.int16 else (-128, 127, ref.POISON8)


def run(dec, received, frames, D, E_max, stride=0, offsets=None, counts=None, mask_bits=None, period=0, shift=0, clamp=None, lead=0):
    """the call through the C ABI on `received` (a numpy array that ends its device allocation) -> the output as a numpy array
    [frames * 3 D], after the whole buffer, the guard behind it and the input have been checked; `lead` elements in front of the output
    put it off a dword boundary"""
    import torch
    lo, hi, poison = limits(received.dtype)
    clamp = (lo, hi) if clamp is None else clamp
    n3 = 3 * D
    d_in = torch.from_numpy(received.copy()).cuda()
    buf = torch.full((lead + frames * n3 + ref.GUARD,), poison, dtype=d_in.dtype, device="cuda")
    u32 = lambda x: None if x is None else torch.from_numpy(np.asarray(x, dtype=np.uint32).view(np.int32)).cuda()     # noqa: E731
    d_off, d_cnt = u32(offsets), u32(counts)
    d_mask = None if mask_bits is None else torch.from_numpy(ref.pack_bits(mask_bits)).cuda()
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())                                                    # noqa: E731
    rc = _lib.load().vit_hip_lte_rate_dematch_batch(
        dec._handle._h, ptr(d_in), received.size, stride, ptr(d_off), ptr(d_cnt), frames, D, E_max, ptr(d_mask), period, shift, clamp[0],
        clamp[1], C.c_void_p(buf.data_ptr() + lead * buf.element_size()), None)
    assert rc == _lib.OK, _lib.load().vit_hip_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lead] == poison).all() and (got[lead + frames * n3:] == poison).all()
    assert np.array_equal(d_in.cpu().numpy(), received)            # the input is only read
    return got[lead:lead + frames * n3]


def full_scale(rng, dtype, n):
    """random elements, a quarter of them at the ends of the range"""
    lo, hi, _ = limits(dtype)
    x = rng.integers(lo, hi + 1, size=n)
    ends = rng.integers(0, 8, size=n)
    x[ends == 0], x[ends == 1] = lo, hi
    return x.astype(dtype)


def check(dec, received, frames, D, E_max, **kw):
    lo, hi, _ = limits(received.dtype)
    clamp = kw.get("clamp") or (lo, hi)
    got = run(dec, received, frames, D, E_max, **kw)
    kw.pop("lead", None), kw.pop("clamp", None)
    want = ref.dematch(received.tolist(), frames, D, E_max, lo=clamp[0], hi=clamp[1], **kw)
    bad = np.flatnonzero(got != np.asarray(want))
    assert bad.size == 0, (D, E_max, frames, kw.get("shift"), "first at", bad[:4], got[bad[:4]], [want[i] for i in bad[:4]])


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("D", DS)
def test_every_length_and_every_count(decode_type, D):
    """3 frames at every E, full-scale inputs: the clamp acts wherever a bit is repeated.  The output starts 0 .. 3 elements behind a dword"""
    _, pc, dec = decoder(decode_type)
    dtype = np.dtype(pc.soft_dtype).type
    rng = np.random.default_rng(D)
    for i, E in enumerate(es(D)):
        if D == 1024 and E == 16 * 3 * D and decode_type != "SOFT16":
            E = 4 * 3 * D + 1                                      # many wraps of the longest frame once; the scalar loop is the cost
        received = full_scale(rng, dtype, 3 * E + 2)
        check(dec, received, 3, D, E, stride=E + 1, shift=(0, 1, 4)[i % 3], lead=i % 4)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
@pytest.mark.parametrize("frames", [1, 300])
def test_one_frame_and_three_hundred(decode_type, frames):
    """a ragged last block, dword groups that straddle two frames (3 D odd), small values so that the sums stay inside the clamp"""
    _, pc, dec = decoder(decode_type)
    dtype = np.dtype(pc.soft_dtype).type
    rng = np.random.default_rng(frames)
    for D, E, shift in ((1, 1, 0), (7, 47, 1), (33, 100, 0), (40, 1920, 4), (43, 72, 0), (43, 576, 1), (65, 194, 4), (64, 200, 0)):
        received = rng.integers(-7, 8, size=frames * E).astype(dtype)
        check(dec, received, frames, D, E, stride=E, shift=shift, lead=(D + frames) % 4)


@pytest.mark.parametrize("shift", [1, 4])
def test_rounding_at_the_boundary_and_below_zero(shift):
    """sums of exactly +-(half), +-(half) +- 1 and +-3 half: D = 1, E = 6, the two elements of an output chosen to give each sum"""
    _, pc, dec = decoder("SOFT16")
    half = (1 << shift) >> 1
    sums = [s * m + d for s in (1, -1) for m in (half, 3 * half, 1 << shift) for d in (-1, 0, 1)]
    frames = -(-len(sums) // 3)
    sums += [0] * (3 * frames - len(sums))
    where = ref.rate_match_map(1)
    received = np.zeros(frames * 6, dtype=np.int16)
    for f in range(frames):
        for k in range(6):
            s = sums[3 * f + where[k % 3]]
            received[6 * f + k] = 1000 if k < 3 else s - 1000
    got = run(dec, received, frames, 1, 6, stride=6, shift=shift)
    assert got.tolist() == [(s + half) >> shift for s in sums]
    assert got.tolist() == ref.dematch(received.tolist(), frames, 1, 6, stride=6, shift=shift)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_placement_offsets_counts_and_the_end_of_the_input(decode_type):
    _, pc, dec = decoder(decode_type)
    dtype = np.dtype(pc.soft_dtype).type
    rng = np.random.default_rng(11)
    D, E_max, n = 43, 576, 2001
    received = full_scale(rng, dtype, n)
    offsets = [0, 1, 73, 145, 144, 0, n - 576, n - 575, n - 1, n, n + 1, 2 ** 32 - 1, 2 ** 31, 999, 7]
    counts = [576, 72, 144, 288, 0, 577, 2 ** 32 - 1, 576, 9, 5, 5, 5, 5, 2 ** 31, 1]
    bits = rng.integers(0, 2, size=n).tolist()
    for kw in (dict(), dict(mask_bits=bits), dict(mask_bits=bits[:576], period=576), dict(mask_bits=bits[:100], period=100)):
        check(dec, received, len(offsets), D, E_max, offsets=offsets, counts=counts, shift=1, clamp=(-100, 90), **kw)
        check(dec, received, len(offsets), D, E_max, offsets=offsets, **kw)
    # a stride above E_max, counts without offsets, one mask for the batch (period = stride) and one for the region
    E, stride, frames = 130, 137, 14
    received = full_scale(rng, dtype, (frames - 1) * stride + E)
    counts = [E, 0, 1, E + 1, 129, 128, 2 ** 32 - 1, 64, 65, 3, E, E, 2, 100]
    bits = rng.integers(0, 2, size=received.size).tolist()
    for kw in (dict(), dict(mask_bits=bits[:stride], period=stride), dict(mask_bits=bits, period=0)):
        check(dec, received, frames, D, E, stride=stride, counts=counts, **kw)
        check(dec, received, frames, 40, E, stride=stride, shift=4, **kw)


def test_a_frame_longer_than_any_on_chip_memory_and_the_int32_sum():
    """D = 8192 (24576 outputs a frame, 48 KiB of int16) in 2 frames, and D = 1 with 66667 full-scale repetitions: the sum wraps"""
    _, pc, dec = decoder("SOFT16")
    rng = np.random.default_rng(13)
    D, E = 8192, 3 * 8192 + 77
    received = rng.integers(-3000, 3000, size=2 * E).astype(np.int16)
    got = run(dec, received, 2, D, E, stride=E, shift=1, lead=1)
    want = lte_rate_dematch_numpy(received, 2, D, E, received_frame_stride=E, shift=1)      # checked against the scalar loop on the CPU
    assert np.array_equal(got, want.reshape(-1))
    assert got[:3 * 300].tolist() == ref.dematch(received.tolist(), 1, D, E, stride=E, shift=1)[:3 * 300]
    received = np.full(200001, 32767, dtype=np.int16)
    assert run(dec, received, 1, 1, 200001, stride=200001).tolist() == [-32768] * 3


def test_rejections_launch_nothing():
    import torch
    L = _lib.load()
    _, pc, dec = decoder("SOFT16")
    _, _, dec8 = decoder("SOFT8")
    code2 = COMMON_CODES[2]
    dec2 = BatchDecoder(*make_table_config(code2, "SOFT16")[1:])
    assert dec2.R == 2
    frames, D, E = 4, 10, 40
    d_in = torch.full((frames * E + 3,), 77, dtype=torch.int16, device="cuda")
    out = torch.full((frames * 3 * D + 8,), ref.POISON16, dtype=torch.int16, device="cuda")
    cnt = torch.zeros(frames, dtype=torch.int32, device="cuda")
    h, a, o = dec._handle._h, d_in.data_ptr(), out.data_ptr()

    def call(hh=h, rec=a, n=frames * E, stride=E, off=None, count=None, fr=frames, D_=D, E_=E, scr=None, period=0, shift=0, lo=-32768, hi=32767,
             out_=o):
        return L.vit_hip_lte_rate_dematch_batch(hh, rec, n, stride, off, count, fr, D_, E_, scr, period, shift, lo, hi, out_, None)

    bad = [dict(hh=None), dict(rec=None), dict(out_=None), dict(hh=dec2._handle._h), dict(D_=0), dict(D_=8193), dict(E_=0), dict(E_=1 << 24),
           dict(n=1 << 32), dict(shift=16), dict(lo=5, hi=4), dict(lo=-32769), dict(hi=32768), dict(hh=dec8._handle._h, hi=128),
           dict(hh=dec8._handle._h, lo=-129, hi=0), dict(stride=E - 1), dict(n=frames * E - 1), dict(stride=E + 1),
           dict(out_=a), dict(out_=a + 2 * frames * E - 2), dict(out_=a - 2 * frames * 3 * D + 2), dict(rec=a + 1), dict(out_=o + 1),
           dict(off=cnt.data_ptr(), out_=cnt.data_ptr()), dict(fr=(1 << 32) // 30 + 1, off=cnt.data_ptr())]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(fr=0) == _lib.OK
    torch.cuda.synchronize()
    assert (out == ref.POISON16).all().item() and (d_in == 77).all().item() and not cnt.any().item()
    assert call(lo=7, hi=7) == _lib.OK and call(n=frames * E + 3, stride=E + 1) == _lib.OK and call(E_=(1 << 24) - 1, off=cnt.data_ptr()) == _lib.OK
    torch.cuda.synchronize()
    assert (out[frames * 3 * D:] == ref.POISON16).all().item()
    received = d_in[:frames * E].view(frames, E)
    for kw in (dict(D=0), dict(D=8193), dict(D=D, E=E + 1), dict(D=D, shift=16), dict(D=D, clamp=(3, 2)), dict(D=D, offsets=cnt),
               dict(D=D, counts=cnt[:3]), dict(D=D, counts=cnt.to(torch.int64)), dict(D=D, out=out[:7]),
               dict(D=D, scramble=torch.zeros(4, dtype=torch.uint8, device="cuda"), scramble_period=E)):
        with pytest.raises(ValueError):
            dec.lte_rate_dematch(received, **kw)
    with pytest.raises(ValueError):
        dec.lte_rate_dematch(received.cpu(), D)
    with pytest.raises(ValueError):
        dec.lte_rate_dematch(received.to(torch.int8), D)
    with pytest.raises(ValueError):
        dec2.lte_rate_dematch(received, D)


def pdcch_blocks(F, seed):
    """F blocks of 27 payload bits + LTE_CRC16 XOR an RNTI -> (the 6 bytes of each, the RNTIs)"""
    rng = np.random.default_rng(seed)
    rnti = rng.integers(1, 1 << 16, size=F)
    payload = rng.integers(0, 256, size=(F, 4), dtype=np.uint8)
    payload[:, 3] &= 0xE0
    return crc_append_numpy(LTE_CRC16, payload, 27, mask=rnti), rnti


def pdcch_regions(dec, pc, sent, levels, seed, noise):
    """the blocks as candidates in shared control regions of 8 CCEs: block b takes candidate b mod C of region b // C, the candidates of
    `levels` being laid side by side inside a region (level by level, so that they do not collide); every region is scrambled with its
    own Gold sequence.  returns (the soft bits of all regions, offsets, counts, the mask bits of all regions, E_max)"""
    import torch
    F, L = sent.shape[0], 43
    rng = np.random.default_rng(seed)
    sym = dec.encode(torch.from_numpy(sent).cuda(), L, tail=False, tail_biting=True).cpu().numpy()
    offs, cnts = [], []
    at = 0
    for Lv in levels:                                              # one candidate of every level, side by side
        offs.append(at), cnts.append(72 * Lv)
        at += 72 * Lv
    region = at
    C_ = len(levels)
    regions = -(-F // C_)
    mid = (pc.soft_decision_high + pc.soft_decision_low) // 2
    soft = np.full(regions * region, mid, dtype=pc.soft_dtype)
    bits = np.concatenate([lte_gold_sequence(1000 + r, region)[1] for r in range(regions)])
    offsets, counts = np.zeros(F, dtype=np.uint32), np.zeros(F, dtype=np.uint32)
    for b in range(F):
        r, c = divmod(b, C_)
        offsets[b], counts[b] = r * region + offs[c], cnts[c]
        soft[offsets[b]:offsets[b] + counts[b]] = lte_rate_match_numpy(sym[b], counts[b])
    if noise:
        soft = np.clip(soft.astype(np.int64) + rng.normal(0, noise, size=soft.size).round().astype(np.int64), pc.soft_decision_low,
                       pc.soft_decision_high).astype(pc.soft_dtype)
    soft = np.where(bits != 0, -soft.astype(np.int64), soft).clip(-32768, 32767).astype(pc.soft_dtype)                 # the scrambler
    return soft, offsets, counts, bits, 72 * max(levels)


def cpu_composition(oracle, code, pc, soft, offsets, counts, bits, D, E_max, shift):
    want_sym = lte_rate_dematch_numpy(soft, len(offsets), D, E_max, offsets=offsets, counts=counts, scramble=np.packbits(bits), shift=shift,
                                      clamp_lo=pc.soft_decision_low, clamp_hi=pc.soft_decision_high)
    want_out, _, _ = tb_reference(oracle, code, oracle_cfg("SOFT16", code.R), want_sym, D)
    return want_sym, want_out, crc_numpy(LTE_CRC16, want_out, 27) ^ crc_field_numpy(LTE_CRC16, want_out, 27)


def gpu_route(dec, soft, offsets, counts, bits, D, E_max, shift):
    import torch
    d_off, d_cnt = (torch.from_numpy(x.view(np.int32)).cuda() for x in (offsets, counts))
    sym = dec.lte_rate_dematch(torch.from_numpy(soft).cuda(), D, E=E_max, offsets=d_off, counts=d_cnt,
                               scramble=torch.from_numpy(np.packbits(bits)).cuda(), shift=shift)
    out = dec.decode_tail_biting(sym, D)
    crc, syn = dec.crc_check(LTE_CRC16, out, 27)
    torch.cuda.synchronize()
    return sym.cpu().numpy(), out.cpu().numpy(), syn.cpu().numpy().view(np.uint32).astype(np.int64)


def test_the_pdcch_route_noise_free_every_syndrome_is_the_rnti(oracle):
    code, pc, dec = decoder("SOFT16")
    sent, rnti = pdcch_blocks(512, 27)
    soft, offsets, counts, bits, E_max = pdcch_regions(dec, pc, sent, (2, 4, 8), 3, 0)
    assert sorted(set(counts.tolist())) == [144, 288, 576]
    sym, out, syn = gpu_route(dec, soft, offsets, counts, bits, 43, E_max, 0)
    assert sym.shape == (512, 43, 3) and np.array_equal(out, sent) and np.array_equal(syn, rnti)
    want_sym, want_out, want_syn = cpu_composition(oracle, code, pc, soft, offsets, counts, bits, 43, E_max, 0)
    assert np.array_equal(sym, want_sym) and np.array_equal(out, want_out) and np.array_equal(syn, want_syn)


@pytest.mark.parametrize("levels,noise", [((1,), 0), ((1,), 150), ((2, 4, 8), 250)], ids=["punctured", "punctured_noisy", "noisy"])
def test_the_pdcch_route_equals_the_cpu_composition(oracle, levels, noise):
    """E = 72 < 3 D, and additive noise: only that the card computes what the CPU composition computes, bit for bit"""
    code, pc, dec = decoder("SOFT16")
    sent, rnti = pdcch_blocks(512, 28)
    soft, offsets, counts, bits, E_max = pdcch_regions(dec, pc, sent, levels, 4, noise)
    sym, out, syn = gpu_route(dec, soft, offsets, counts, bits, 43, E_max, 1 if noise else 0)
    want_sym, want_out, want_syn = cpu_composition(oracle, code, pc, soft, offsets, counts, bits, 43, E_max, 1 if noise else 0)
    assert np.array_equal(sym, want_sym) and np.array_equal(out, want_out) and np.array_equal(syn, want_syn)
    print("blocks decoded as sent:", int((out == sent).all(axis=1).sum()), "of", len(sent))


@pytest.mark.parametrize("noise", [0, 400])
def test_pbch_sixteen_repetitions_added(oracle, noise):
    """D = 40, E = 1920, the cell's mask shared by the batch (period E), shift 4: the mean of the 16 repetitions"""
    import torch
    code, pc, dec = decoder("SOFT16")
    F, D, E = 64, 40, 1920
    rng = np.random.default_rng(40)
    mask16 = rng.integers(0, 1 << 16, size=F)
    payload = rng.integers(0, 256, size=(F, 3), dtype=np.uint8)
    sent = crc_append_numpy(LTE_CRC16, payload, 24, mask=mask16)
    sym0 = dec.encode(torch.from_numpy(sent).cuda(), D, tail=False, tail_biting=True).cpu().numpy()
    soft = lte_rate_match_numpy(sym0, E).astype(np.int64)
    if noise:
        soft = soft + rng.normal(0, noise, size=soft.shape).round().astype(np.int64)
    packed, bits = lte_gold_sequence(301, E)
    soft = np.where(bits != 0, -soft, soft).clip(-32768, 32767).astype(pc.soft_dtype)
    sym = dec.lte_rate_dematch(torch.from_numpy(soft).cuda(), D, scramble=torch.from_numpy(packed).cuda(), scramble_period=E, shift=4)
    out = dec.decode_tail_biting(sym, D)
    crc, syn = dec.crc_check(LTE_CRC16, out, 24)
    torch.cuda.synchronize()
    want_sym = lte_rate_dematch_numpy(soft.reshape(-1), F, D, E, received_frame_stride=E, scramble=packed, scramble_period=E, shift=4,
                                      clamp_lo=pc.soft_decision_low, clamp_hi=pc.soft_decision_high)
    assert want_sym[:2].reshape(-1).tolist() == ref.dematch(soft[:2].reshape(-1).tolist(), 2, D, E, stride=E, mask_bits=bits.tolist(), period=E,
                                                           shift=4, lo=pc.soft_decision_low, hi=pc.soft_decision_high)
    want_out, _, _ = tb_reference(oracle, code, oracle_cfg("SOFT16", code.R), want_sym, D)
    assert np.array_equal(sym.cpu().numpy(), want_sym) and np.array_equal(out.cpu().numpy(), want_out)
    got_syn = syn.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(got_syn, crc_numpy(LTE_CRC16, want_out, 24) ^ crc_field_numpy(LTE_CRC16, want_out, 24))
    if not noise:
        assert np.array_equal(sym.cpu().numpy(), sym0) and np.array_equal(out.cpu().numpy(), sent) and np.array_equal(got_syn, mask16)


def test_captured_into_a_graph_alone_and_with_the_decode_and_the_check():
    import torch
    code, pc, dec = decoder("SOFT16")
    F, D = 48, 43
    offsets, counts = pdcch_candidates(8, levels=(2, 4, 8))
    offsets, counts = np.tile(offsets, F // len(offsets) + 1)[:F], np.tile(counts, F // len(counts) + 1)[:F]
    rng = np.random.default_rng(9)
    inputs, wants = [], []
    for trial in range(2):
        sent, rnti = pdcch_blocks(F, 50 + trial)
        sym = dec.encode(torch.from_numpy(sent).cuda(), D, tail=False, tail_biting=True).cpu().numpy()
        region = np.zeros((F, 576), dtype=np.int16)                # one region a block: its candidate at its offset, noise elsewhere
        region[:] = rng.integers(-100, 100, size=region.shape)
        for b in range(F):
            region[b, offsets[b]:offsets[b] + counts[b]] = lte_rate_match_numpy(sym[b], counts[b])
        inputs.append(region.reshape(-1))
        wants.append((sent, rnti, sym))
    where = (np.arange(F) * 576 + offsets).astype(np.uint32)
    d_in = torch.from_numpy(inputs[0]).cuda()
    d_off, d_cnt = (torch.from_numpy(x.view(np.int32)).cuda() for x in (where, counts))
    d_sym = torch.empty((F, D, 3), dtype=torch.int16, device="cuda")
    d_out = torch.empty((F, 6), dtype=torch.uint8, device="cuda")
    d_crc, d_syn = (torch.empty(F, dtype=torch.int32, device="cuda") for _ in range(2))
    ws = torch.empty(dec.tail_biting_workspace_bytes(F, D), dtype=torch.uint8, device="cuda")

    def dematch():
        dec.lte_rate_dematch(d_in, D, E=576, offsets=d_off, counts=d_cnt, out=d_sym)

    def chain():
        dematch()
        dec.decode_tail_biting(d_sym, D, out=d_out, workspace=ws)
        dec.crc_check(LTE_CRC16, d_out, 27, crc_out=d_crc, syndrome_out=d_syn)

    for body, whole in ((dematch, False), (chain, True)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()                                                 # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        for flat, (sent, rnti, sym) in zip(inputs, wants):
            d_in.copy_(torch.from_numpy(flat).cuda())
            d_sym.fill_(ref.POISON16), d_out.fill_(0xA5), d_syn.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(d_sym.cpu().numpy(), sym)
            if whole:
                assert np.array_equal(d_out.cpu().numpy(), sent)
                assert np.array_equal(d_syn.cpu().numpy().view(np.uint32).astype(np.int64), rnti)
