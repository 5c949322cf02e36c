"""DAB+ superframes on the GPU: vit_hip_dabplus_sync / vit_hip_dabplus_au_batch and their Python layer against the restatement of
tests/dabplus_reference.py (a bit-serial shift register for both CRCs, the header bit by bit).  Every element of every output buffer is
compared, written or not: outputs are pre-filled with a canary and carry a guard behind them.
The AU kernel gives an access unit one wave of 64 lanes with right-aligned chunks of C = dabplus_chunk_bytes(s) bytes, 64 C >= 110 s: the
"chunk times group" length 64 C is therefore never below the longest access unit a superframe can hold (110 s - 10), and the cases around
it are the longest access unit itself; lengths one below, at and one above C and 2 C, 3 C are all reached."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, DABPLUS_RS_120_110, BatchDecoder, DabPlusDecoder, _lib, dab_energy_dispersal_numpy,
                                   dab_puncture_numpy, dab_time_interleave_numpy, dabplus_au_table_numpy, dabplus_superframe_numpy,
                                   dabplus_sync_numpy, eep_profile, frames_extract_numpy, rs_decode_numpy, rs_encode_numpy, synth)
from tests import dabplus_reference as ref
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

GUARD = 32
CANARY = 0xA5A5A5A5
SYNC_BLOCK = 256                                                   # frames of one block of the sync kernel
FORMATS = [(0, 1), (1, 1), (0, 0), (1, 0)]


@functools.lru_cache(maxsize=None)
def decoder():
    code = COMMON_CODES[4]
    pc, table, config = make_table_config(code, "SOFT16")
    return code, pc, BatchDecoder(table, config)


def ptr(x, offset=0):
    return None if x is None else C.c_void_p(x.data_ptr() + offset)


def u32(values):
    import torch
    return None if values is None else torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def words(x):
    return x.cpu().numpy().view(np.uint32).reshape(-1).tolist()


def chunk_bytes(s):
    return ((110 * s + 63) // 64 + 3) & ~3


# ---- sync ------------------------------------------------------------------------------------------------------------------------------

def hit_frame(rng, fb):
    f = rng.integers(0, 256, size=fb).tolist()
    c = ref.shift_register(f, 2, 9, 0x782F, 0)
    f[0], f[1] = c >> 8, c & 255
    return f


def make_frames(rng, rows, F, fb, hit_phase=None, frame0=0):
    """random frames; with hit_phase [rows], the frames of that phase of row r carry a right Fire code"""
    return [[hit_frame(rng, fb) if hit_phase is not None and (frame0 + f) % 5 == hit_phase[r] else rng.integers(0, 256, size=fb).tolist()
             for f in range(F)] for r in range(rows)]


def call_sync(frames, fb, counts=None, frame0=0, totals=None, lead=0, frame_stride=0, row_pad=0, want_lock=True, max_frames=None):
    """the raw ABI on frames [rows][F] of byte lists; returns (rc, hits, count, lock) as flat uint32 lists, guard included"""
    import torch
    _, _, dec = decoder()
    rows, F = len(frames), len(frames[0])
    fs = frame_stride or fb
    rs = F * fs + row_pad
    image = np.full(lead + rows * rs + 8, 0x3C, dtype=np.uint8)
    for r in range(rows):
        for f in range(F):
            image[lead + r * rs + f * fs:lead + r * rs + f * fs + fb] = frames[r][f]
    d_in = torch.from_numpy(image).cuda()
    fill = (lambda n, t: torch.from_numpy(np.concatenate([np.asarray(t, dtype=np.uint32).reshape(-1), np.full(GUARD, CANARY, dtype=np.uint32)])
                                          .view(np.int32).copy()).cuda() if t is not None else u32([CANARY] * (n + GUARD)))
    hits, count = fill(rows * 5, None if totals is None else totals[0]), fill(rows * 5, None if totals is None else totals[1])
    lock = u32([CANARY] * (rows * 4 + GUARD))
    rc = _lib.load().vit_hip_dabplus_sync(dec._handle._h, ptr(d_in, lead), rs if (row_pad or frame_stride) else 0, frame_stride, fb, rows,
                                          F if max_frames is None else max_frames, ptr(u32(counts)), frame0,
                                          _lib.MARKER_ACCUMULATE if totals is not None else 0, ptr(hits), ptr(count),
                                          ptr(lock) if want_lock else None, dec._stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), image)
    return rc, words(hits), words(count), words(lock)


def check_sync(frames, fb, counts=None, frame0=0, totals=None, **kw):
    rc, hits, count, lock = call_sync(frames, fb, counts, frame0, totals, **kw)
    assert rc == 0, _lib.load().vit_hip_last_error()
    want = ref.sync_image(frames, counts, frame0, fb, *([] if totals is None else totals))
    flat = lambda x: [v for row in x for v in row]                 # noqa: E731
    assert hits == flat(want[0]) + [CANARY] * GUARD and count == flat(want[1]) + [CANARY] * GUARD
    assert lock == flat(want[2]) + [CANARY] * GUARD
    return want


@pytest.mark.parametrize("fb", [24, 11, 72])
@pytest.mark.parametrize("F", [1, 4, 5, 6, 11, SYNC_BLOCK + 3])
def test_sync_frame_sizes_and_counts(fb, F):
    rng = np.random.default_rng(100 * fb + F)
    for frame0 in range(5):
        frames = make_frames(rng, 3, F, fb, hit_phase=[1, 4, 0], frame0=frame0)
        want = check_sync(frames, fb, counts=[F, 0, F + 9], frame0=frame0, lead=frame0 % 4, frame_stride=fb + (frame0 % 3), row_pad=frame0)
        if F >= 5:
            assert [lk[0] for lk in want[2]] == [8 * fb, 0, 0] and want[2][1][2:] == [0, 0] and want[2][2][2] == 0
    check_sync(make_frames(rng, 1, F, fb, hit_phase=[2]), fb)     # one row, no counts, packed


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_sync_at_every_base_alignment(lead):
    rng = np.random.default_rng(lead)
    check_sync(make_frames(rng, 2, 13, 24, hit_phase=[3, 1]), 24, lead=lead)
    check_sync(make_frames(rng, 2, 13, 11, hit_phase=[3, 1]), 11, lead=lead, frame_stride=13)


def test_sync_cut_into_two_accumulating_calls():
    rng = np.random.default_rng(7)
    frames = make_frames(rng, 2, 10, 24, hit_phase=[2, 0], frame0=3)
    whole = check_sync(frames, 24, frame0=3)
    for cut in range(1, 10):
        first = check_sync([row[:cut] for row in frames], 24, frame0=3)
        second = check_sync([row[cut:] for row in frames], 24, frame0=(3 + cut) % 5, totals=(first[0], first[1]))
        assert second == whole


def test_sync_zero_frames_flips_a_tie_and_no_hit():
    rng = np.random.default_rng(8)
    frames = make_frames(rng, 1, 10, 24, hit_phase=[1])
    frames[0][6] = [0] * 24                                        # an all-zero header checks trivially: no hit
    assert check_sync(frames, 24)[0] == [[0, 1, 0, 0, 0]]
    good = hit_frame(rng, 24)
    for byte in range(12):
        broken = list(good)
        broken[byte] ^= 1 << (byte % 8)
        assert ref.fire_hit(broken) == (byte == 11)
        assert check_sync([[broken]], 24)[0] == [[1 if byte == 11 else 0, 0, 0, 0, 0]]
    tie = make_frames(rng, 1, 10, 24)
    tie[0][3], tie[0][9] = hit_frame(rng, 24), hit_frame(rng, 24)  # phases 3 and 4, one hit of two each
    assert check_sync(tie, 24)[2] == [[3 * 192, 0, 1, 2]]
    none = check_sync(make_frames(rng, 2, 7, 24), 24)
    assert none[2] == [[0, 0, 2, 2], [0, 0, 2, 2]]
    rc, hits, count, lock = call_sync(make_frames(rng, 1, 5, 24, hit_phase=[2]), 24, want_lock=False)
    assert rc == 0 and hits[:5] == [0, 0, 1, 0, 0] and lock == [CANARY] * (4 + GUARD)


# ---- AU table --------------------------------------------------------------------------------------------------------------------------

def superframe(rng, dac, sbr, s, fixed=(), starts=None, low=0):
    n, first = ref.FORMATS[(dac, sbr)]
    aus = [rng.integers(0, 256, size=L).tolist() for L in ref.split_lengths(110 * s - first, n, rng, fixed=fixed)]
    return ref.build_data(aus, dac, sbr, s, low, starts) + rng.integers(0, 256, size=10 * s).tolist()


def call_au(sfs, s, counts=None, status=None, stride=0, lead=0, max_frames=None):
    """the raw ABI on superframes [rows][F] of 120 s byte lists; returns (rc, info, au) as flat uint32 lists, guard included"""
    import torch
    _, _, dec = decoder()
    rows, F = len(sfs), len(sfs[0])
    st = stride or 120 * s
    image = np.full(lead + rows * F * st + 8, 0x3C, dtype=np.uint8)
    for r in range(rows):
        for f in range(F):
            at = lead + (r * F + f) * st
            image[at:at + min(st, 120 * s)] = sfs[r][f][:min(st, 120 * s)]
    d_in = torch.from_numpy(image).cuda()
    info, au = u32([CANARY] * (rows * F + GUARD)), u32([CANARY] * (rows * F * 18 + GUARD))
    d_status = None if status is None else torch.from_numpy(np.asarray(status, dtype=np.int32).reshape(-1).copy()).cuda()
    rc = _lib.load().vit_hip_dabplus_au_batch(dec._handle._h, ptr(d_in, lead), stride, rows, F if max_frames is None else max_frames,
                                              ptr(u32(counts)), s, ptr(d_status), ptr(info), ptr(au), dec._stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), image)
    return rc, words(info), words(au)


def check_au(sfs, s, counts=None, status=None, **kw):
    rc, info, au = call_au(sfs, s, counts, status, **kw)
    assert rc == 0, _lib.load().vit_hip_last_error()
    want = ref.au_image(sfs, counts, s, status, CANARY)
    assert info == want[0] + [CANARY] * GUARD and au == want[1] + [CANARY] * GUARD
    return want


@pytest.mark.parametrize("s", [1, 2, 7, 24])
def test_au_table_formats_lengths_and_alignments(s):
    rng = np.random.default_rng(s)
    Cb = chunk_bytes(s)
    assert 64 * Cb >= 110 * s > 64 * (Cb - 4)
    row = [superframe(rng, dac, sbr, s, low=i) for i, (dac, sbr) in enumerate(FORMATS)]
    row.append(superframe(rng, 0, 1, s, fixed=(1,)))               # an access unit of one data byte; the other fills the superframe
    row.append(superframe(rng, 0, 1, s, fixed=(110 * s - 5 - 2 - 3,)))           # the longest access unit there is, then one byte
    for L in (Cb - 1, Cb, Cb + 1, 2 * Cb - 1, 2 * Cb, 2 * Cb + 1, 3 * Cb):      # around the chunk and its multiples; the starts behind them
        if L + 31 <= 110 * s:                                                   # run through every residue mod 4
            row.append(superframe(rng, 1, 0, s, fixed=(L, 1 + L % 3)))
    for L in (1, 2, 3, 4):
        row.append(superframe(rng, 0, 0, s, fixed=(L,)))
    want = check_au([row], s, lead=s % 4)
    assert all(v & 3 == 3 for v in want[0]) and all(v == 0 for v in want[1][2::3][:2])
    starts = {want[1][3 * i] % 4 for i in range(len(want[1]) // 3) if want[1][3 * i + 1]}
    assert starts == {0, 1, 2, 3}


def test_au_table_broken_crc_fire_code_and_status():
    rng = np.random.default_rng(50)
    s = 2
    row = [superframe(rng, 1, 0, s) for _ in range(4)]
    at = ref.header(row[0], s)[3]
    row[0][at[3]] ^= 0x80                                          # the first data byte of access unit 3
    row[1][0] ^= 0x40                                              # the Fire code
    status = [[[0, 0], [1, 2], [5, -1], [0, 0]]]
    want = check_au([row], s, status=status)
    assert [i for i in range(6) if want[1][3 * i + 2]] == [3] and want[0][1] & 1 == 0 and want[1][18:36] == list(ref.EMPTY) * 6
    assert [v >> 2 & 1 for v in want[0]] == [0, 0, 1, 0]
    assert [v >> 2 & 1 for v in check_au([row], s)[0]] == [0, 0, 0, 0]


@pytest.mark.parametrize("s", [1, 24])
def test_au_table_hostile_headers(s):
    rng = np.random.default_rng(60 + s)
    row = []
    for dac, sbr in FORMATS:
        n, first = ref.FORMATS[(dac, sbr)]
        for starts in ([first + 3] * (n - 1), [110 * s - 3 - k for k in range(n - 1)], [first + 2 + 3 * k for k in range(n - 1)],
                       [110 * s + 1 + 3 * k for k in range(n - 1)], [0xFFF] * (n - 1), [110 * s - 2] * (n - 1)):
            row.append(superframe(rng, dac, sbr, s, starts=starts))
    want = check_au([row], s)
    # (0, 1) has one field: first + 3 and 110 s - 3 are consistent there; everything else is not
    assert [v & 3 for v in want[0]] == [3, 3, 1, 1, 1, 1] + [1] * 18


def test_au_table_counts_rows_and_stride():
    rng = np.random.default_rng(70)
    s = 3
    sfs = [[superframe(rng, *FORMATS[(r + f) % 4], s) for f in range(4)] for r in range(3)]
    check_au(sfs, s, counts=[2, 0, 9])
    check_au(sfs, s, counts=[4, 1, 3], stride=120 * s + 7, lead=1, status=rng.integers(-1, 3, size=(3, 4, s)).tolist())
    check_au(sfs, s, stride=110 * s)                               # the data alone


# ---- rejections ------------------------------------------------------------------------------------------------------------------------

def test_every_rejection_leaves_the_outputs_untouched():
    import torch
    _, _, dec = decoder()
    L, h = _lib.load(), dec._handle._h
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    hits, count, lock, info, au = (u32([CANARY] * 64) for _ in range(5))
    nf = u32([1, 1])
    P, st = ptr, dec._stream()

    def sync(h=h, d=buf, rs=0, fs=0, fb=24, rows=2, mf=4, n=nf, f0=0, flags=0, hi=hits, co=count, lo=lock, off=0):
        return L.vit_hip_dabplus_sync(h, P(d), rs, fs, fb, rows, mf, P(n, off), f0, flags, P(hi), P(co), P(lo), st)

    def table(h=h, d=buf, stride=0, rows=2, mf=2, n=nf, s=2, rs=None, i=info, a=au, off=0):
        return L.vit_hip_dabplus_au_batch(h, P(d), stride, rows, mf, P(n), s, P(rs), P(i, off), P(a), st)

    bad = [sync(h=None), sync(d=None), sync(hi=None), sync(co=None), sync(flags=2), sync(fb=10), sync(fb=(1 << 31) // 40 + 1), sync(f0=5),
           sync(fs=23), sync(rs=95), sync(rows=1 << 31), sync(mf=1 << 31), sync(off=2), sync(co=hits), sync(lo=hits), sync(hi=buf.view(torch.int32)),
           table(h=None), table(d=None), table(i=None), table(a=None), table(s=0), table(s=25), table(stride=219), table(rows=1 << 31),
           table(mf=1 << 31), table(rows=(1 << 31) - 1, mf=(1 << 31) - 1), table(off=2), table(a=info), table(i=buf.view(torch.int32))]
    torch.cuda.synchronize()
    assert bad == [_lib.ERR_INVALID_ARG] * len(bad)
    for x in (hits, count, lock, info, au):
        assert words(x) == [CANARY] * 64
    assert not buf.any()
    assert sync(rows=0) == 0 and table(rows=0) == 0 and table(mf=0) == 0 and sync(mf=0, lo=None) == 0
    torch.cuda.synchronize()
    assert words(hits)[:12] == [0] * 10 + [CANARY] * 2 and words(info) == [CANARY] * 64
    with pytest.raises(ValueError):
        dec.dabplus_sync(buf.view(4, 1024)[:, :10])
    with pytest.raises(ValueError):
        dec.dabplus_sync(buf.view(4, 1024), frame_bytes=24, frame0=5)
    with pytest.raises(ValueError):
        dec.dabplus_au_table(buf.view(4, 1024), 25)
    with pytest.raises(ValueError):
        dec.dabplus_au_table(buf.view(4, 1024)[:, :109], 1)


# ---- the chain at byte level ---------------------------------------------------------------------------------------------------------------

S_CHAIN, ROWS_CHAIN, CUTS = 2, 2, (1, 7, 5, 10)


@functools.lru_cache(maxsize=None)
def chain_stream(seed):
    """2 rows of 23 logical frames that start at superframe position 3: 5 byte errors in every codeword of superframe 1, 6 in codeword 0
    of superframe 2 (row 0) -- uint8 [rows][23][24 s]"""
    rng = np.random.default_rng(seed)
    s, B = S_CHAIN, 24 * S_CHAIN
    rows = []
    for r in range(ROWS_CHAIN):
        sfs = []
        for i in range(6):
            dac, sbr = FORMATS[(i + r) % 4]
            n, first = ref.FORMATS[(dac, sbr)]
            aus = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in ref.split_lengths(110 * s - first, n, rng)]
            sf = dabplus_superframe_numpy(aus, dac, sbr, s, byte2_low=i).reshape(-1)
            for c in range(s):
                k = 5 if i == 2 else (6 if (i == 3 and c == 0 and r == 0) else 0)
                if k:
                    sf[c + s * rng.choice(120, size=k, replace=False)] ^= rng.integers(1, 256, size=k).astype(np.uint8)
            sfs.append(sf.reshape(5, B))
        rows.append(np.concatenate(sfs)[3:26])
    return np.stack(rows)


def host_chain(stream, cuts):
    """the composition of the numpy rules, push by push: a list of (superframes [rows][k][120 s] with 0xEE where not written, n_frames,
    info, au, status) with the canary where not written"""
    s, B = S_CHAIN, 24 * S_CHAIN
    rows = stream.shape[0]
    totals, carry, carry_bits, emitted, at, out = None, [None] * rows, [0] * rows, 0, 0, []
    for cut in cuts:
        part = stream[:, at:at + cut]
        hits, count, lock = dabplus_sync_numpy(part, frame0=emitted % 5, totals=totals)
        totals = (hits, count)
        k = -(-cut * 8 * B // (40 * B))
        sf = np.full((rows, k, 120 * s), 0xEE, dtype=np.uint8)
        nf = np.zeros(rows, dtype=np.int64)
        info = np.full((rows, k), CANARY, dtype=np.int64)
        au = np.full((rows, k, 6, 3), CANARY, dtype=np.int64)
        status = np.full((rows, k, s), CANARY, dtype=np.int64)
        for r in range(rows):
            got, _, carry[r], carry_bits[r] = frames_extract_numpy(part[r].reshape(-1), cut * 8 * B, 40 * B, (emitted % 5) * 8 * B, lock[r], carry[r],
                                                                   carry_bits[r])
            nf[r] = got.shape[0]
            if nf[r]:
                sf[r, :nf[r]], status[r, :nf[r]] = rs_decode_numpy(DABPLUS_RS_120_110, got, s)
                info[r, :nf[r]], au[r, :nf[r]] = dabplus_au_table_numpy(sf[r, :nf[r]], s, status[r, :nf[r]])
        out.append((sf, nf, info, au, status & 0xFFFFFFFF))
        emitted, at = emitted + cut, at + cut
    return out


def test_the_chain_at_byte_level():
    import torch
    _, _, dec = decoder()
    s, B = S_CHAIN, 24 * S_CHAIN
    stream = chain_stream(3)
    want = host_chain(stream, CUTS)
    # what the rule gives: the first superframe starts at frame 2; a superframe is delivered by the push that brings its last frame
    ends = np.cumsum(CUTS)
    assert [int(w[1][0]) for w in want] == [sum(1 for j in range(4) if (lo < 2 + 5 * (j + 1) <= hi)) for lo, hi in zip([0] + ends[:-1].tolist(), ends)]
    assert sum(int(w[1][0]) for w in want) == (23 - 2) // 5 == 4
    totals = tuple(torch.zeros(shape, dtype=torch.int32, device="cuda") for shape in ((2, 5), (2, 5), (2, 4)))
    cb = (40 * B * 8 // 8 - 1 + 7) // 8
    carry = [torch.zeros((2, cb), dtype=torch.uint8, device="cuda") for _ in range(2)]
    carry_bits = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2)]
    at = emitted = 0
    for i, cut in enumerate(CUTS):
        part = torch.from_numpy(stream[:, at:at + cut].copy()).cuda()
        dec.dabplus_sync(part, frame0=emitted % 5, out=totals, accumulate=True)
        k = dec.frames_capacity(cut * 8 * B, 40 * B)
        sf = torch.full((2, k, 120 * s), 0xEE, dtype=torch.uint8, device="cuda")
        nf = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        dec.frames_extract(part.view(2, cut * B), cut * 8 * B, 40 * B, (emitted % 5) * 8 * B, totals[2], carry[i % 2], carry_bits[i % 2],
                           max_frames=k, out=(sf, nf, None, carry[1 - i % 2], carry_bits[1 - i % 2]))
        status = u32([CANARY] * (2 * k * s)).view(2, k, s)
        dec.rs_decode(DABPLUS_RS_120_110, sf, nf, interleave=s, status=status)
        info, au = u32([CANARY] * (2 * k)).view(2, k), u32([CANARY] * (2 * k * 18)).view(2, k, 6, 3)
        dec.dabplus_au_table(sf, s, nf, status, out=(info, au))
        torch.cuda.synchronize()
        w = want[i]
        assert np.array_equal(sf.cpu().numpy(), w[0]) and nf.tolist() == w[1].tolist()
        assert words(info) == w[2].reshape(-1).tolist() and words(au) == w[3].reshape(-1).tolist() and words(status) == w[4].reshape(-1).tolist()
        at, emitted = at + cut, emitted + cut
    # superframe 1 of the stream (index 2 of the six) is delivered by the third push, superframe 2 (index 3) by the fourth as its first
    assert (want[2][4][:, 0] == 5).all() and (want[2][3][:, 0, :, 2] % (1 << 32) != 0).sum() == (want[2][3][:, 0, :, 2] == 0xFFFFFFFF).sum()
    assert want[3][2][0, 0] & 4 and want[3][4][0, 0].tolist() == [0xFFFFFFFF, 0] and not want[3][2][1, 0] & 4
    assert np.array_equal(want[3][0][0, 0, 0::2], stream[0, 12:17].reshape(-1)[0::2])      # codeword 0 as received


def test_the_chain_in_one_graph():
    import torch
    _, _, dec = decoder()
    s, B, F = S_CHAIN, 24 * S_CHAIN, 23
    k = dec.frames_capacity(F * 8 * B, 40 * B)
    d_in = torch.zeros((2, F, B), dtype=torch.uint8, device="cuda")
    totals = tuple(torch.zeros(shape, dtype=torch.int32, device="cuda") for shape in ((2, 5), (2, 5), (2, 4)))
    sf = torch.zeros((2, k, 120 * s), dtype=torch.uint8, device="cuda")
    nf, cbits = (torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2))
    carry = torch.zeros((2, 120 * s), dtype=torch.uint8, device="cuda")
    status = torch.zeros((2, k, s), dtype=torch.int32, device="cuda")
    info, au = torch.zeros((2, k), dtype=torch.int32, device="cuda"), torch.zeros((2, k, 6, 3), dtype=torch.int32, device="cuda")

    def chain():
        dec.dabplus_sync(d_in, out=totals)
        dec.frames_extract(d_in.view(2, F * B), F * 8 * B, 40 * B, 0, totals[2], max_frames=k, out=(sf, nf, None, carry, cbits))
        dec.rs_decode(DABPLUS_RS_120_110, sf, nf, interleave=s, status=status)
        dec.dabplus_au_table(sf, s, nf, status, out=(info, au))

    def results():
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (totals[0], totals[1], totals[2], sf, nf, status, info, au)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                    # warm-up outside the capture: the code's tables are uploaded here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for seed in (11, 12):
        stream = chain_stream(seed)
        d_in.copy_(torch.from_numpy(stream).cuda())
        for x in (sf, status, info, au):
            x.fill_(0x5A)
        graph.replay()
        replayed = results()
        for x in (sf, status, info, au):
            x.fill_(0x5A)
        chain()
        eager = results()
        assert all(np.array_equal(a, b) for a, b in zip(replayed, eager))
        w = host_chain(stream, (F,))[0]
        assert replayed[4].tolist() == [4, 4] and np.array_equal(replayed[3][:, :4], w[0][:, :4])
        assert np.array_equal(replayed[6][:, :4].view(np.uint32), w[2][:, :4]) and np.array_equal(replayed[7][:, :4].view(np.uint32), w[3][:, :4])
        assert (replayed[6][:, 4:] == 0x5A).all() and (replayed[7][:, 4:] == 0x5A).all()          # behind the count: the fill


# ---- from soft bits ------------------------------------------------------------------------------------------------------------------------

def test_from_soft_bits_to_checked_access_units():
    import torch
    code, pc, dec = decoder()
    profile = eep_profile("3-A", 1)
    s = profile.info_bits // 192
    rows, B = 2, 24 * s
    rng = np.random.default_rng(21)
    logical, sent = [], []
    for r in range(rows):
        frames, aus_sent = [rng.integers(0, 256, size=(2, B), dtype=np.uint8)], []     # superframes start at logical frame 2
        for i in range(5):
            dac, sbr = FORMATS[(i + r) % 4]
            n, first = ref.FORMATS[(dac, sbr)]
            aus = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in ref.split_lengths(110 * s - first, n, rng)]
            aus_sent.append(aus)
            frames.append(dabplus_superframe_numpy(aus, dac, sbr, s))
        logical.append(np.concatenate(frames + [rng.integers(0, 256, size=(1, B), dtype=np.uint8)]))
        sent.append(aus_sent)
    logical = np.stack(logical)                                    # [rows][28][B]: 13 behind the 15 the de-interleaver holds back
    assert logical.shape == (rows, 28, B)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, dab_energy_dispersal_numpy(logical).reshape(rows * 28, B))
    sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, None, code.R, rng, pc.soft_dtype)
    kept = dab_puncture_numpy(sym, profile).reshape(rows, 28, profile.n_received)
    tx = torch.from_numpy(np.stack([dab_time_interleave_numpy(kept[r]) for r in range(rows)])).cuda()
    rx = DabPlusDecoder(dec, profile, rows=rows)
    assert rx.s == s
    got, at = [[] for _ in range(rows)], 0
    for cut in (4, 13, 3, 8):                                      # 28 sent: 13 logical frames come out, frames 0 .. 12
        sf, nf, info, au, status = rx.push(tx[:, at:at + cut])
        at += cut
        torch.cuda.synchronize()
        sf, nf, info, au = sf.cpu().numpy(), nf.tolist(), info.cpu().numpy().view(np.uint32), au.cpu().numpy().view(np.uint32)
        for r in range(rows):
            for f in range(nf[r]):
                got[r].append((sf[r, f], int(info[r, f]), au[r, f]))
    assert rx.emitted == 13 and rx.lock.cpu().numpy()[:, 0].tolist() == [2 * 8 * B] * rows
    for r in range(rows):
        assert len(got[r]) == 2                                    # frames 2 .. 11: the first two superframes
        for i, (sf, info, au) in enumerate(got[r]):
            n = len(sent[r][i])
            assert info & 7 == 3 and info >> 4 & 15 == n
            for k in range(n):
                start, nb, syn = (int(v) for v in au[k])
                assert syn == 0 and sf[start:start + nb].tolist() == sent[r][i][k].tolist()
    import types
    for bits in (200, 192 * 25, 0):
        with pytest.raises(ValueError):
            DabPlusDecoder(dec, types.SimpleNamespace(info_bits=bits), rows=1)
