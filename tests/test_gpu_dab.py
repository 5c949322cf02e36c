"""The DAB receive chain on the GPU: vit_hip_dab_deinterleave_batch / vit_hip_dab_descramble_batch and their Python layer against the
restatement of tests/dab_reference.py (per-residue FIFOs, a walk along the puncturing vectors, a 9-bit shift register).  Every byte of
every output is compared, written or not: outputs are pre-filled with a sentinel and carry a guard behind them.  n_received {1, 15, 16,
17, 100, 256} with the identity map, the 4-A, 3-A, 2-A and 1-B profiles at n = 1, a map with out-of-range and negative entries; nf {0, 1,
14, 15, 16, 17, 40} x fill {0, 1, 14, 15, 99}; one call against the same frames cut 1 + 14 + 1 + 24; 1 and 3 rows with per-row counts,
one above max_frames; reading in place at strides above n_received; SOFT16, SOFT8 and HARD8 handles; the dispersal at n_bits {0, 1, 7, 8,
9, 511, 512, 768, 1025, 6144} in place and out of place with strides, rows and counts; every rejection; both calls in one graph around
decode; the sub-channel route on a clean and on a noisy channel against the CPU composition of restatement and oracle; the FIC route."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, DAB_CRC16, FIC_PROFILE, BatchDecoder, DabSubchannelDecoder, _lib, crc_append_numpy,
                                   dab_energy_dispersal_numpy, dab_puncture_numpy, dab_time_interleave_numpy, eep_profile, synth)
from tests import dab_reference as ref
from tests.helpers import make_table_config, oracle_cfg

pytestmark = pytest.mark.gpu

GUARD = 64
H = 15


@functools.lru_cache(maxsize=None)
def decoder(decode_type="SOFT16"):
    code = COMMON_CODES[4]
    assert (code.name, code.K, code.R) == ("DAB Radio", 7, 4)
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config)


def poison_of(dtype):
    return ref.POISON16 if np.dtype(dtype) == np.int16 else ref.POISON8


def ptr(x, offset_elements=0):
    return None if x is None else C.c_void_p(x.data_ptr() + offset_elements * x.element_size())


def u32(values):
    import torch
    return None if values is None else torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def call_deinterleave(dec, frames, counts=None, hists=None, fills=None, idx=None, frame_stride=0, row_stride=0, lead=0, hist_stride=0):
    """one call through the C ABI -> (out [rows][mf][spf], n_out, hist_out [rows][15 n], fill_out) as numpy arrays, after every byte of
    every output buffer has been compared with the image of the restatement and the inputs with what was uploaded.
    frames: [rows][mf][n]; with frame_stride / row_stride (elements) they are embedded in a larger buffer of other values and read in
    place; `lead` elements in front of the output put it off a dword boundary"""
    import torch
    rows, mf, n = frames.shape
    dtype = frames.dtype
    poison = poison_of(dtype)
    fs = frame_stride or n
    rs = row_stride or mf * fs
    rng = np.random.default_rng(rows * 100 + mf)
    host_in = rng.integers(-100, 100, size=(rows - 1) * rs + (mf - 1) * fs + n).astype(dtype)
    for r in range(rows):
        for f in range(mf):
            host_in[r * rs + f * fs:r * rs + f * fs + n] = frames[r, f]
    d_in = torch.from_numpy(host_in.copy()).cuda()
    spf = n if idx is None else len(idx)
    d_idx = None if idx is None else torch.from_numpy(np.asarray(idx, dtype=np.int64).astype(np.int32)).cuda()
    hs = hist_stride or H * n
    d_hist = None
    if hists is not None:
        host_hist = rng.integers(-100, 100, size=(rows, hs)).astype(dtype)
        host_hist[:, :H * n] = np.asarray(hists, dtype=dtype).reshape(rows, H * n)
        d_hist = torch.from_numpy(host_hist.copy()).cuda()
    d_cnt, d_fill = u32(counts), u32(fills)
    out = torch.full((lead + rows * mf * spf + GUARD,), poison, dtype=d_in.dtype, device="cuda")
    hist_out = torch.full((rows * hs + GUARD,), poison, dtype=d_in.dtype, device="cuda")
    n_out, fill_out = (torch.from_numpy(np.full(rows + 2, ref.POISON_COUNT, dtype=np.uint32).view(np.int32)).cuda() for _ in range(2))
    rc = _lib.load().vit_hip_dab_deinterleave_batch(
        dec._handle._h, ptr(d_in), row_stride, frame_stride, rows, mf, ptr(d_cnt), n, ptr(d_idx), spf, ptr(d_hist), ptr(d_fill), hist_stride,
        ptr(out, lead), ptr(n_out), ptr(hist_out), ptr(fill_out), None)
    assert rc == _lib.OK, _lib.load().vit_hip_last_error()
    torch.cuda.synchronize()
    want_out, want_n, want_hist, want_fill = ref.deinterleave_image(
        frames.tolist(), counts, None if hists is None else np.asarray(hists).reshape(rows, H, n).tolist(), fills, n, mf, idx, poison)
    got = out.cpu().numpy()
    assert (got[:lead] == poison).all() and (got[lead + rows * mf * spf:] == poison).all()
    got = got[lead:lead + rows * mf * spf]
    bad = np.flatnonzero(got != np.asarray(want_out, dtype=np.int64).astype(dtype))
    assert bad.size == 0, ("out differs first at", bad[:4], got[bad[:4]])
    got_hist = hist_out.cpu().numpy()
    assert (got_hist[rows * hs:] == poison).all()
    got_hist = got_hist[:rows * hs].reshape(rows, hs)
    assert (got_hist[:, H * n:] == poison).all()
    assert np.array_equal(got_hist[:, :H * n], np.asarray(want_hist, dtype=np.int64).astype(dtype))
    got_n, got_fill = n_out.cpu().numpy().view(np.uint32), fill_out.cpu().numpy().view(np.uint32)
    assert got_n[:rows].tolist() == want_n and got_fill[:rows].tolist() == want_fill
    assert (got_n[rows:] == ref.POISON_COUNT).all() and (got_fill[rows:] == ref.POISON_COUNT).all()
    assert np.array_equal(d_in.cpu().numpy(), host_in)             # the input is only read
    return got.reshape(rows, mf, spf), got_n[:rows].copy(), got_hist[:, :H * n].copy(), got_fill[:rows].copy()


def soft(rng, dtype, shape):
    """random soft bits over the whole range of the type, none equal to the sentinel's low byte pattern by construction of the check"""
    lo, hi = (-32768, 32767) if np.dtype(dtype) == np.int16 else (-128, 127)
    return rng.integers(lo, hi + 1, size=shape).astype(dtype)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 100, 256])
def test_every_length_with_the_identity_map(decode_type, n):
    _, pc, dec = decoder(decode_type)
    rng = np.random.default_rng(n)
    frames = soft(rng, pc.soft_dtype, (1, 18, n))
    out, n_out, _, _ = call_deinterleave(dec, frames, lead=n % 4)
    assert n_out[0] == 3
    assert np.array_equal(out[0, 0], frames[0, np.asarray([ref.delay(i) for i in range(n)]), np.arange(n)])


@pytest.mark.parametrize("decode_type,level", [("SOFT16", "4-A"), ("SOFT16", "3-A"), ("SOFT16", "2-A"), ("SOFT16", "1-B"), ("SOFT8", "4-A"),
                                               ("HARD8", "4-A")])
def test_the_profiles(decode_type, level):
    _, pc, dec = decoder(decode_type)
    p = eep_profile(level, 1)
    if level == "4-A":
        assert (p.n_received, p.symbols_per_frame) == (256, 792)
    rng = np.random.default_rng(len(level) + p.n_received)
    frames = soft(rng, pc.soft_dtype, (1, 17, p.n_received))
    idx, kept = ref.source_map(ref.mask_walk(p.segments))
    assert kept == p.n_received and idx == p.source_index().tolist()
    out, n_out, _, _ = call_deinterleave(dec, frames, idx=idx, lead=1)
    assert n_out[0] == 2 and (out[0, :2][:, ~p.mask()] == 0).all()


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_a_map_with_out_of_range_and_negative_entries(decode_type):
    _, pc, dec = decoder(decode_type)
    rng = np.random.default_rng(8)
    n = 100
    idx = rng.integers(-5, n + 10, size=77).tolist()
    idx[:8] = [-1, n, n - 1, 0, -2 ** 31, 2 ** 31 - 1, n + 1, 16]
    frames = soft(rng, pc.soft_dtype, (2, 20, n))
    out, n_out, _, _ = call_deinterleave(dec, frames, idx=idx, lead=3)
    assert n_out.tolist() == [5, 5] and (out[:, :5, [0, 1, 4, 5, 6]] == 0).all()


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
@pytest.mark.parametrize("nf", [0, 1, 14, 15, 16, 17, 40])
def test_every_count_against_every_fill(decode_type, nf):
    """five rows, one fill each; the history rows hold 15 frames whatever their fill says"""
    _, pc, dec = decoder(decode_type)
    rng = np.random.default_rng(nf)
    n, fills = 17, [0, 1, 14, 15, 99]
    frames = soft(rng, pc.soft_dtype, (5, 40, n))
    hists = soft(rng, pc.soft_dtype, (5, H * n))
    _, n_out, _, fill_out = call_deinterleave(dec, frames, counts=[nf] * 5, hists=hists, fills=fills, lead=nf % 2)
    assert n_out.tolist() == [max(0, min(f, H) + nf - H) for f in fills]
    assert fill_out.tolist() == [min(H, min(f, H) + nf) for f in fills]


def test_one_call_against_the_same_frames_cut_into_four():
    _, pc, dec = decoder("SOFT16")
    rng = np.random.default_rng(40)
    n = 100
    logical = soft(rng, np.int16, (40, n))
    sent = dab_time_interleave_numpy(logical)
    assert sent.tolist() == ref.interleave(logical.tolist())
    whole, n_out, hist, fill = call_deinterleave(dec, sent[None])
    assert n_out[0] == 25 and fill[0] == 15 and np.array_equal(whole[0, :25], logical[:25]) and np.array_equal(hist[0], sent[25:].reshape(-1))
    hist, fill, got, at = None, None, [], 0
    for c in (1, 14, 1, 24):
        out, n_out, hist, fill = call_deinterleave(dec, sent[None, at:at + c], hists=hist, fills=None if fill is None else fill.tolist())
        got.append(out[0, :n_out[0]])
        at += c
    assert np.array_equal(np.concatenate(got), logical[:25])


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("rows", [1, 3])
def test_rows_counts_and_reading_in_place(decode_type, rows):
    """per-row counts, one above max_frames; frames read in place at a frame stride above n_received and a row stride above the frames;
    a history with a row stride of its own; a map, so that output frames are no multiple of a dword"""
    _, pc, dec = decoder(decode_type)
    rng = np.random.default_rng(rows)
    n, mf = 33, 21
    idx = [i if i % 5 else -1 for i in range(n)] + [7, 8, 9]
    frames = soft(rng, pc.soft_dtype, (rows, mf, n))
    hists = soft(rng, pc.soft_dtype, (rows, H * n))
    counts, fills = [mf + 5, 3, 0][:rows], [15, 14, 2][:rows]
    _, n_out, _, _ = call_deinterleave(dec, frames, counts=counts, hists=hists, fills=fills, idx=idx, frame_stride=n + 7, row_stride=mf * (n + 7) + 5,
                                       hist_stride=H * n + 3, lead=rows)
    assert n_out.tolist() == [mf, 2, 0][:rows]
    call_deinterleave(dec, frames, counts=counts, frame_stride=55, lead=2)


# ---- energy dispersal ---------------------------------------------------------------------------------------------------------------

def call_descramble(dec, frames, n_bits, counts=None, in_place=False, out_stride=0, lead=0):
    """frames: uint8 [rows][mf][stride] -> the call through the C ABI, every byte of the output buffer compared with its image"""
    import torch
    rows, mf, stride = frames.shape
    nb = (n_bits + 7) // 8
    d_cnt = u32(counts)
    buf = torch.full((lead + frames.size + GUARD,), ref.POISON_BYTE, dtype=torch.uint8, device="cuda")
    buf[lead:lead + frames.size] = torch.from_numpy(frames.reshape(-1).copy()).cuda()
    if in_place:
        os_, out, before = stride, buf, frames.reshape(-1).tolist()
        out_lead = lead
    else:
        os_ = out_stride or nb
        out_lead = (lead + 1) % 4
        out = torch.full((out_lead + rows * mf * os_ + GUARD,), ref.POISON_BYTE, dtype=torch.uint8, device="cuda")
        before = None
    rc = _lib.load().vit_hip_dab_descramble_batch(dec._handle._h, ptr(buf, lead), stride, rows, mf, ptr(d_cnt), n_bits, ptr(out, out_lead),
                                                  stride if in_place else out_stride, None)
    assert rc == _lib.OK, _lib.load().vit_hip_last_error()
    torch.cuda.synchronize()
    want = ref.descramble_image(frames.tolist(), counts, n_bits, mf, os_, before=before)
    got = out.cpu().numpy()
    assert (got[:out_lead] == ref.POISON_BYTE).all() and (got[out_lead + rows * mf * os_:] == ref.POISON_BYTE).all()
    got = got[out_lead:out_lead + rows * mf * os_]
    bad = np.flatnonzero(got != np.asarray(want, dtype=np.uint8))
    assert bad.size == 0, (n_bits, in_place, "first at", bad[:4])
    if not in_place:
        assert np.array_equal(buf.cpu().numpy()[lead:lead + frames.size], frames.reshape(-1))
    return got.reshape(rows, mf, os_)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n_bits", [0, 1, 7, 8, 9, 511, 512, 768, 1022 + 3, 6144])
def test_the_dispersal_at_every_length(n_bits, in_place):
    _, _, dec = decoder("SOFT16")
    rng = np.random.default_rng(n_bits)
    nb = (n_bits + 7) // 8
    for rows, mf, extra, counts, lead in ((1, 5, 0, None, 0), (3, 4, 3, [4, 9, 1], 1), (2, 3, 1, [0, 2], 2), (1, 70, 0, [69], 3)):
        if n_bits == 6144 and mf == 70:
            mf = 9
            counts = [8]
        frames = rng.integers(0, 256, size=(rows, mf, nb + extra), dtype=np.uint8)
        got = call_descramble(dec, frames, n_bits, counts=counts, in_place=in_place, out_stride=0 if extra == 0 else nb + 2, lead=lead)
        if n_bits and counts is None:
            assert np.array_equal(got[..., :nb], dab_energy_dispersal_numpy(frames, n_bits))


def test_the_python_layer_of_the_dispersal():
    import torch
    _, _, dec = decoder("SOFT16")
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, size=(2, 6, 100), dtype=np.uint8)
    d = torch.from_numpy(x).cuda()
    got = dec.dab_descramble(d, 768)
    assert got.shape == (2, 6, 96) and np.array_equal(got.cpu().numpy(), dab_energy_dispersal_numpy(x, 768))
    cnt = torch.tensor([2, 6], dtype=torch.int32, device="cuda")
    again = dec.dab_descramble(d, 799, n_frames=cnt, in_place=True)
    assert again is d
    want = x.copy()
    want[0, :2], want[1] = dab_energy_dispersal_numpy(x[0, :2], 799), dab_energy_dispersal_numpy(x[1], 799)
    assert np.array_equal(d.cpu().numpy(), want)
    for bad in (lambda: dec.dab_descramble(d, -1), lambda: dec.dab_descramble(d, 801), lambda: dec.dab_descramble(d, 8, out=d, in_place=True),
                lambda: dec.dab_descramble(d, 8, out=torch.empty((2, 5, 1), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            bad()


# ---- rejections -----------------------------------------------------------------------------------------------------------------------

def test_every_rejection_leaves_the_outputs_untouched():
    import torch
    _, _, dec = decoder("SOFT16")
    lib, h = _lib.load(), dec._handle._h
    n, mf, rows, spf = 32, 4, 2, 40
    big = torch.full((4096,), ref.POISON16, dtype=torch.int16, device="cuda")
    d_in, d_hist = big[:rows * mf * n], big[512:512 + rows * H * n]
    out = torch.full((rows * mf * spf,), ref.POISON16, dtype=torch.int16, device="cuda")
    hist_out = torch.full((rows * H * n,), ref.POISON16, dtype=torch.int16, device="cuda")
    cnts = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n_out, fill_out, fill_in, n_frames = cnts[0:2], cnts[2:4], cnts[4:6], cnts[6:8]
    idx = torch.zeros(spf, dtype=torch.int32, device="cuda")
    good = dict(h=h, d_in=ptr(d_in), rs=0, fs=0, rows=rows, mf=mf, nfr=ptr(n_frames), n=n, idx=ptr(idx), spf=spf, hist=ptr(d_hist), fill=ptr(fill_in),
                hs=0, out=ptr(out), n_out=ptr(n_out), hist_out=ptr(hist_out), fill_out=ptr(fill_out))

    def deint(**kw):
        a = dict(good, **kw)
        return lib.vit_hip_dab_deinterleave_batch(a["h"], a["d_in"], a["rs"], a["fs"], a["rows"], a["mf"], a["nfr"], a["n"], a["idx"], a["spf"],
                                                  a["hist"], a["fill"], a["hs"], a["out"], a["n_out"], a["hist_out"], a["fill_out"], None)

    bad = [dict(h=None), dict(d_in=None), dict(out=None), dict(n_out=None), dict(hist_out=None), dict(fill_out=None), dict(fill=None),
           dict(n=0), dict(spf=0), dict(fs=n - 1), dict(rs=mf * n - 1), dict(fs=n + 1, rs=mf * (n + 1) - 1), dict(hs=H * n - 1),
           dict(idx=None), dict(idx=None, spf=n + 1), dict(n=2 ** 28), dict(spf=2 ** 32),
           dict(d_in=ptr(d_in, 0).value + 1), dict(out=out.data_ptr() + 1), dict(hist=d_hist.data_ptr() + 1), dict(hist_out=hist_out.data_ptr() + 1),
           dict(idx=idx.data_ptr() + 2), dict(n_out=n_out.data_ptr() + 2), dict(nfr=n_frames.data_ptr() + 1),
           dict(out=ptr(d_in)), dict(out=ptr(d_hist)), dict(out=ptr(hist_out)), dict(out=ptr(idx)), dict(hist_out=ptr(d_in)),
           dict(hist_out=ptr(d_hist)), dict(hist_out=ptr(idx)), dict(n_out=ptr(n_frames)), dict(n_out=ptr(fill_in)), dict(fill_out=ptr(n_frames)),
           dict(fill_out=ptr(fill_in)), dict(fill_out=ptr(n_out)), dict(rows=2 ** 31), dict(mf=2 ** 31, fs=n), dict(rows=2 ** 20, mf=2 ** 20),
           dict(rows=2 ** 13, mf=2 ** 14, spf=2 ** 5, idx=ptr(idx))]
    for kw in bad:
        kw = {k: (C.c_void_p(v) if isinstance(v, int) and k in ("d_in", "out", "hist", "hist_out", "idx", "n_out", "nfr") else v) for k, v in kw.items()}
        assert deint(**kw) == _lib.ERR_INVALID_ARG, kw
        assert lib.vit_hip_last_error()
    assert deint(rows=0) == _lib.OK and deint(mf=0) == _lib.OK

    frames = torch.full((rows * mf * 12,), 0x5A, dtype=torch.uint8, device="cuda")
    dout = torch.full((rows * mf * 12,), 0x5A, dtype=torch.uint8, device="cuda")
    gd = dict(h=h, d_in=ptr(frames), s=0, rows=rows, mf=mf, nfr=ptr(n_frames), bits=90, out=ptr(dout), os=0)

    def descr(**kw):
        a = dict(gd, **kw)
        return lib.vit_hip_dab_descramble_batch(a["h"], a["d_in"], a["s"], a["rows"], a["mf"], a["nfr"], a["bits"], a["out"], a["os"], None)

    for kw in (dict(h=None), dict(d_in=None), dict(out=None), dict(bits=2 ** 32 - 33), dict(s=11), dict(os=11), dict(rows=2 ** 31), dict(mf=2 ** 31),
               dict(rows=2 ** 16, mf=2 ** 15), dict(out=ptr(frames), os=13), dict(out=ptr(frames, 1)), dict(out=ptr(frames, 12)),
               dict(out=ptr(cnts.view(torch.uint8), 24))):
        assert descr(**kw) == _lib.ERR_INVALID_ARG, kw
    assert descr(rows=0) == _lib.OK and descr(mf=0) == _lib.OK and descr(bits=0) == _lib.OK
    torch.cuda.synchronize()
    for x in (big, out, hist_out):
        assert (x.cpu().numpy() == ref.POISON16).all()
    assert (cnts.cpu().numpy() == 0x5A5A5A5A).all()
    assert (frames.cpu().numpy() == 0x5A).all() and (dout.cpu().numpy() == 0x5A).all()


def test_the_rules_of_the_python_layer():
    import torch
    _, _, dec = decoder("SOFT16")
    x = torch.zeros((2, 20, 64), dtype=torch.int16, device="cuda")
    out, n_out, hist, fill = dec.dab_deinterleave(x)
    assert out.shape == (2, 20, 64) and n_out.tolist() == [5, 5] and fill.tolist() == [15, 15] and hist.shape == (2, 15 * 64)
    view = torch.zeros((2, 20, 100), dtype=torch.int16, device="cuda")[:, :, 10:74]          # a sub-channel inside larger frames
    out2 = dec.dab_deinterleave(view, hist=hist, fill=fill)
    assert out2[1].tolist() == [20, 20]
    for bad in (lambda: dec.dab_deinterleave(x.to(torch.int8)), lambda: dec.dab_deinterleave(x, hist=hist), lambda: dec.dab_deinterleave(x[:, :0]),
                lambda: dec.dab_deinterleave(x, hist=hist, fill=fill, out=(out, n_out, hist, fill)),
                lambda: dec.dab_deinterleave(x, source_index=torch.zeros(4, dtype=torch.int64, device="cuda")),
                lambda: dec.dab_deinterleave(x.transpose(1, 2))):
        with pytest.raises(ValueError):
            bad()


# ---- graphs and whole chains ----------------------------------------------------------------------------------------------------------

def transmit(code, pc, profile, rows, cifs, seed, ebn0_db=None):
    """random bytes -> dispersal -> the encoder -> puncturing -> the time interleaver: (data [rows][cifs][I/8], sent [rows][cifs][n_received])"""
    rng = np.random.default_rng(seed)
    nb = profile.info_bits // 8
    data = rng.integers(0, 256, size=(rows, cifs, nb), dtype=np.uint8)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, dab_energy_dispersal_numpy(data).reshape(rows * cifs, nb))
    sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, ebn0_db, code.R, rng, pc.soft_dtype)
    kept = dab_puncture_numpy(sym, profile).reshape(rows, cifs, profile.n_received)
    return data, np.stack([dab_time_interleave_numpy(kept[r]) for r in range(rows)])


def cpu_composition(oracle, code, decode_type, profile, sent):
    """the restatement's FIFOs and depuncturing, the oracle's decode, the restatement's shift register: bytes [rows][cifs - 15][I/8]"""
    mask = ref.mask_walk(profile.segments)
    out = []
    for row in sent:
        logical = ref.fifo_deinterleave(row.tolist(), profile.n_received)
        sym = np.asarray([ref.depuncture(fr, mask) for fr in logical], dtype=sent.dtype).reshape(len(logical), profile.steps, 4)
        dec, _, _ = oracle.decode_frames(code.K, code.R, code.G, oracle_cfg(decode_type, code.R), sym, profile.info_bits)
        out.append([ref.descramble_frame(fr.tolist(), profile.info_bits) for fr in dec])
    return np.asarray(out, dtype=np.uint8)


@pytest.mark.parametrize("decode_type,ebn0_db", [("SOFT16", None), ("SOFT16", 3.0), ("SOFT8", 4.0)])
def test_the_sub_channel_route(oracle, decode_type, ebn0_db):
    import torch
    code, pc, dec = decoder(decode_type)
    profile = eep_profile("3-A", 1)
    rows, cifs = 2, 40
    data, sent = transmit(code, pc, profile, rows, cifs, seed=77, ebn0_db=ebn0_db)
    cifs_buffer = torch.zeros((rows, cifs, profile.n_received + 40), dtype=dec._soft_dtype, device="cuda")
    cifs_buffer[:, :, 8:8 + profile.n_received] = torch.from_numpy(sent).cuda()
    rx = DabSubchannelDecoder(dec, profile, rows=rows)
    got, at = [], 0
    for c in (7, 9, 24):
        out = rx.push(cifs_buffer[:, at:at + c, 8:8 + profile.n_received])          # read in place
        assert out.shape == (rows, max(0, min(at, H) + c - H), profile.info_bits // 8)
        got.append(out.cpu().numpy())
        at += c
    got = np.concatenate(got, axis=1)
    assert got.shape[1] == 25 and rx.fill == 15
    if ebn0_db is None:
        assert np.array_equal(got, data[:, :25])                   # frames 0 .. 24 exactly
    want = cpu_composition(oracle, code, decode_type, profile, sent)
    assert np.array_equal(got, want)
    rx.reset()
    assert rx.push(cifs_buffer[:, :15, 8:8 + profile.n_received]).shape[1] == 0 and rx.push(torch.from_numpy(sent[:, 15:17]).cuda()).shape[1] == 2


def fic_blocks(frames, seed):
    """FIC blocks of 768 bits: three FIBs of 30 bytes and their CRC-16 each"""
    rng = np.random.default_rng(seed)
    fibs = crc_append_numpy(DAB_CRC16, rng.integers(0, 256, size=(frames, 3, 30), dtype=np.uint8), 240)
    assert fibs.shape == (frames, 3, 32)
    return fibs.reshape(frames, 96)


def test_the_fic_route():
    import torch
    code, pc, dec = decoder("SOFT16")
    F = 20
    blocks = fic_blocks(F, 5)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, dab_energy_dispersal_numpy(blocks))
    sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, None, 4, None, pc.soft_dtype)
    received = torch.from_numpy(dab_puncture_numpy(sym, FIC_PROFILE)).cuda()
    assert received.shape == (F, 2304)
    symbols = dec.depuncture(received, FIC_PROFILE.mask())
    decoded = dec.decode(symbols, FIC_PROFILE.info_bits)
    fibs = dec.dab_descramble(decoded, FIC_PROFILE.info_bits)
    crc, syndrome = dec.crc_check(DAB_CRC16, fibs.view(F * 3, 32), n_bits=240)
    torch.cuda.synchronize()
    assert np.array_equal(fibs.cpu().numpy(), blocks)
    assert (syndrome.cpu().numpy() == 0).all() and crc.shape == (F * 3,)
    broken = fibs.clone()
    broken[3, 40] ^= 1
    _, syndrome = dec.crc_check(DAB_CRC16, broken.view(F * 3, 32), n_bits=240)
    assert np.flatnonzero(syndrome.cpu().numpy()).tolist() == [3 * 3 + 1]


def test_both_calls_in_one_graph_around_the_decode(oracle):
    import torch
    code, pc, dec = decoder("SOFT16")
    profile = eep_profile("4-A", 1)
    rows, cifs = 3, 20
    cases = [transmit(code, pc, profile, rows, cifs, seed=s, ebn0_db=e) for s, e in ((1, None), (2, 4.0))]
    idx = torch.from_numpy(profile.source_index()).cuda()
    d_in = torch.empty((rows, cifs, profile.n_received), dtype=torch.int16, device="cuda")
    sym = torch.empty((rows, cifs, profile.symbols_per_frame), dtype=torch.int16, device="cuda")
    n_out, fill_out = (torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(2))
    hist_out = torch.empty((rows, H * profile.n_received), dtype=torch.int16, device="cuda")
    decoded = torch.empty((rows * cifs, profile.info_bits // 8), dtype=torch.uint8, device="cuda")
    clear = torch.empty((rows, cifs, profile.info_bits // 8), dtype=torch.uint8, device="cuda")

    def chain():
        dec.dab_deinterleave(d_in, source_index=idx, out=(sym, n_out, hist_out, fill_out))
        dec.decode(sym.view(rows * cifs, profile.steps, 4), profile.info_bits, out=decoded)      # every frame: those not completed decode the fill
        dec.dab_descramble(decoded.view(rows, cifs, -1), profile.info_bits, n_frames=n_out, out=clear)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sym.zero_()
        chain()                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for data, sent in cases:
        d_in.copy_(torch.from_numpy(sent).cuda())
        sym.fill_(0), clear.fill_(0xA5), n_out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert n_out.tolist() == [5] * rows and fill_out.tolist() == [15] * rows
        got = clear.cpu().numpy()
        assert (got[:, 5:] == 0xA5).all()
        assert np.array_equal(got[:, :5], cpu_composition(oracle, code, "SOFT16", profile, sent)[:, :5])
        assert np.array_equal(hist_out.cpu().numpy().reshape(rows, H, -1), sent[:, 5:])
