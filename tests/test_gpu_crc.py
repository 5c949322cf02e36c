"""The frame check on the GPU: vit_hip_crc_batch / BatchDecoder.crc_check against the polynomial long division of tests/crc_reference.py.
Widths {1, 5, 8, 16, 24, 31, 32} x every length at which the kernel takes another path (0, 1, around a byte, around the width, around a
32-bit word and two, both sides of every length at which the host rule doubles the lanes of a frame, 8904 = a CCSDS depth-5 frame's
data, 32771) x first_bit {0, 1, 7, 8, 13}, in batches of 1 x 1, 3 x 2 and 1 x 300 (several frames in a wave, a ragged last wave), at an
odd base address and stride, with and without the field; both outputs compared WHOLE over a 0xA5 fill; counts of 0, a part and above
max_frames; the seven catalogue values; every rejection; frames_extract + rs_decode + crc_check in one graph; 512 PDCCH-like blocks
through the tail-biting decoder, the syndrome being the RNTI; and the CCSDS chain through StreamDecoder and MultiStreamDecoder with a
frame Reed-Solomon cannot fault."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (CCSDS_ASM, CCSDS_CRC16, CCSDS_RS_255_223_DUAL, COMMON_CODES, LTE_CRC16, STOCK_CRC_CODES, BatchDecoder,
                                   MultiStreamDecoder, StreamDecoder, _lib, crc_append_numpy, crc_field_numpy, crc_numpy, frame_sync,
                                   rs_encode_numpy, synth)
from tests import crc_reference as ref
from tests import rs_cases
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

POISON32 = int(np.array([ref.POISON32], dtype=np.uint32).view(np.int32)[0])


@functools.lru_cache(maxsize=None)
def decoder(index=2):
    code = COMMON_CODES[index]
    pc, table, config = make_table_config(code, "SOFT16")
    return code, pc, BatchDecoder(table, config)


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def u32(x):
    return x.cpu().numpy().view(np.uint32).astype(np.int64)


def run(case, through_python=True):
    """a case of crc_reference.make_case on the card -> (crc, syndrome) as int64 arrays [rows][max_frames], both whole over the fill
    (syndrome: the untouched fill without field).  The frames lie at the case's odd base address and stride, the last ends the buffer"""
    import torch
    dec = decoder()[2]
    rows, mf, stride, need = case["rows"], case["max_frames"], case["stride"], case["need"]
    raw = torch.from_numpy(case["buffer"].copy()).cuda()
    frames = torch.as_strided(raw, (rows, mf, need), (mf * stride, stride, 1), case["lead"])
    crc = torch.full((rows, mf), POISON32, dtype=torch.int32, device="cuda")
    syn = torch.full((rows, mf), POISON32, dtype=torch.int32, device="cuda")
    counts = None                                                  # uint32 values in int32 storage
    if case["counts"] is not None:
        counts = torch.from_numpy(np.array(case["counts"], dtype=np.uint32).view(np.int32)).cuda()
    if rows * mf == 1:
        frames = frames[0]                                         # [max_frames][stride]: one row
    got = dec.crc_check(case["code"], frames, case["n_bits"], case["first_bit"], counts, field=case["field"], crc_out=crc,
                        syndrome_out=syn if case["field"] else None)
    torch.cuda.synchronize()
    assert (got[0] is crc and got[1] is syn) if case["field"] else got is crc
    assert np.array_equal(raw.cpu().numpy(), case["buffer"])       # the input is only read
    return u32(crc), u32(syn)


def check(case):
    crc, syn = run(case)
    what = (case["code"], case["n_bits"], case["first_bit"], case["rows"], case["max_frames"], case["field"])
    assert np.array_equal(crc, case["crc"]), what
    assert np.array_equal(syn, case["syndrome"]), what


def lengths(width):
    return sorted(set(ref.N_BITS + ref.N_BITS_G + (width - 1, width)))


@pytest.mark.parametrize("width", ref.WIDTHS_GPU)
def test_every_width_length_and_alignment(width):
    """3 rows x 2 frames: every length x every first_bit, with the field; the base address and the stride change with the shape"""
    for n_bits in lengths(width):
        for first_bit in ref.FIRST_BITS:
            check(ref.make_case(width, n_bits, first_bit, 3, 2, True, lead=1 + (n_bits + first_bit) % 4, slack=(n_bits + width) % 5))


@pytest.mark.parametrize("width", ref.WIDTHS_GPU)
def test_one_frame_and_without_the_field(width):
    """1 x 1, and crc alone: a frame then ends with its data, the byte behind is not the kernel's to read"""
    for n_bits in lengths(width):
        for first_bit in (0, 13):
            check(ref.make_case(width, n_bits, first_bit, 1, 1, first_bit == 0, lead=3, slack=0))
            check(ref.make_case(width, n_bits, first_bit, 3, 2, False, lead=2, slack=1))


@pytest.mark.parametrize("width", ref.WIDTHS_GPU)
def test_three_hundred_frames_in_ragged_waves(width):
    """1 x 300: 64 / G frames in a wave, the last wave and the last block partly filled, at every group size"""
    for n_bits in (0, 7, 43, 65, 129, 240, 264, 520, 1032, 2056, 4104, 8904):
        check(ref.make_case(width, n_bits, (n_bits + width) % 14, 1, 300, True, lead=1, slack=1 + n_bits % 3))


@pytest.mark.parametrize("counts", [(0, 0, 0), (2, 0, 5), (7, 300, 6), (0xFFFFFFFF, 3, 1 << 31)], ids=["none", "part", "above", "huge"])
def test_frames_at_or_past_the_count_are_not_written(counts):
    """3 rows of 7 frames: a count of 0, a part, max_frames itself and above it; the entries behind a count keep the fill"""
    for width, n_bits, first_bit in ((16, 43, 0), (24, 8904, 5), (31, 240, 13)):
        case = ref.make_case(width, n_bits, first_bit, 3, 7, True, counts=counts)
        assert ((case["crc"] == ref.POISON32).sum(axis=1) == [7 - min(c, 7) for c in counts]).all()      # width < 32: no CRC is the fill
        check(case)


def test_the_catalogue_on_the_card():
    import torch
    dec = decoder()[2]
    msg = torch.from_numpy(np.frombuffer(b"123456789", dtype=np.uint8).copy()).cuda()[None]
    want = dict(CCSDS_CRC16=0x29B1, LTE_CRC16=0x31C3, DAB_CRC16=0xD64E, LTE_CRC24A=0xCDE703, LTE_CRC24B=0x23EF52, LTE_CRC8=0xEA,
                MPEG2_CRC32=0x0376E6E7)
    assert sorted(want) == sorted(STOCK_CRC_CODES)
    for name, value in want.items():
        crc = dec.crc_check(STOCK_CRC_CODES[name], msg, 72, field=False)
        assert crc.dtype == torch.int32 and tuple(crc.shape) == (1,) and int(u32(crc)[0]) == value, name
    # a FIB: 30 data bytes and the CRC-16 behind them at stride 32; 2 rows of 3
    rng = np.random.default_rng(3)
    fibs = crc_append_numpy(STOCK_CRC_CODES["DAB_CRC16"], rng.integers(0, 256, size=(2, 3, 30), dtype=np.uint8), 240)
    fibs[1, 2, 4] ^= 0x10
    crc, syn = dec.crc_check(STOCK_CRC_CODES["DAB_CRC16"], torch.from_numpy(fibs).cuda(), 240)
    assert tuple(syn.shape) == (2, 3) and (u32(syn) != 0).tolist() == [[False] * 3, [False, False, True]]
    assert np.array_equal(u32(crc), crc_numpy(STOCK_CRC_CODES["DAB_CRC16"], fibs, 240))


def test_rejections_launch_nothing():
    import torch
    L, dec = _lib.load(), decoder()[2]
    rows, mf, stride = 2, 3, 8
    buf = torch.full((rows * mf * stride,), ref.POISON, dtype=torch.uint8, device="cuda")
    outs = torch.full((2 * rows * mf + 1,), POISON32, dtype=torch.int32, device="cuda")
    h, a, c, s = dec._handle._h, buf.data_ptr(), outs.data_ptr(), outs.data_ptr() + 4 * rows * mf
    good = _lib.VitHipCrcParams(16, 0x1021, 0xFFFF, 0)
    P = _lib.VitHipCrcParams

    def call(hh=h, code=good, frames=a, stride_=stride, rows_=rows, mf_=mf, first=0, n=40, crc=c, syn=s):
        return L.vit_hip_crc_batch(hh, None if code is None else C.byref(code), frames, stride_, rows_, mf_, None, first, n, crc, syn, None)

    bad = [dict(hh=None), dict(code=None), dict(frames=None), dict(crc=None, syn=None),
           dict(code=P(0, 0, 0, 0)), dict(code=P(33, 1, 0, 0)), dict(code=P(8, 0x100, 0, 0)), dict(code=P(8, 1, 0x100, 0)), dict(code=P(8, 1, 0, 0x100)),
           dict(code=P(31, 0x80000000, 0, 0)),
           dict(stride_=6), dict(n=49), dict(first=9), dict(stride_=4, syn=None),                # 40 + 16 bits need 7 bytes, 40 alone 5
           dict(syn=c), dict(syn=c + 4 * rows * mf - 4), dict(crc=a), dict(syn=a + rows * mf * stride - 4), dict(crc=a - 4 * rows * mf + 1),
           dict(rows_=1 << 31), dict(mf_=1 << 31), dict(rows_=(1 << 31) - 1, mf_=(1 << 31) - 1, crc=None), dict(n=1 << 32), dict(first=1 << 32)]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(rows_=0) == _lib.OK and call(mf_=0) == _lib.OK
    torch.cuda.synchronize()
    assert (buf == ref.POISON).all().item() and (outs == POISON32).all().item()
    assert call(stride_=7) == _lib.OK and call(stride_=5, syn=None) == _lib.OK and call(stride_=0, n=48) == _lib.OK     # the edges that pass
    torch.cuda.synchronize()
    frames3 = buf.view(rows, mf, stride)
    for kw in (dict(n_bits=49), dict(n_bits=40, first_bit=9), dict(n_bits=-1), dict(n_bits=8, first_bit=-1),
               dict(n_bits=8, n_frames=torch.zeros(3, dtype=torch.int32, device="cuda")),
               dict(n_bits=8, n_frames=torch.zeros(2, dtype=torch.int64, device="cuda")),
               dict(n_bits=8, crc_out=torch.zeros(5, dtype=torch.int32, device="cuda")),
               dict(n_bits=8, syndrome_out=torch.zeros(6, dtype=torch.int32)),
               dict(n_bits=8, field=False, syndrome_out=torch.zeros(6, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            dec.crc_check(CCSDS_CRC16, frames3, **kw)
    with pytest.raises(ValueError):
        dec.crc_check(CCSDS_CRC16, frames3.cpu(), 8)
    with pytest.raises(ValueError):
        dec.crc_check(CCSDS_CRC16, frames3[..., ::2], 8)


def test_frames_extract_rs_decode_and_crc_check_captured_into_a_graph():
    """one chain: the extraction writes the frames and their count, the decode corrects them, the check reads both; replayed on two inputs"""
    import torch
    dec = decoder()[2]
    code, I = rs_cases.CODES["short"], 2
    P, d = 32 + 8 * code.n * I, 32
    data_bits = 8 * (code.k * I - 2)
    pad = frame_sync.ccsds_randomizer(code.n * I)
    n_frames = 4
    rng = np.random.default_rng(8)
    rows, wants = [], []
    for lead in (100, 777):
        payload = crc_append_numpy(CCSDS_CRC16, rng.integers(0, 256, size=(n_frames, code.k * I - 2), dtype=np.uint8), data_bits)
        payload[1, 3] ^= 0x04                                      # a frame whose FECF does not fit, in front of the RS encoder
        sent = rs_encode_numpy(code, payload, I)
        got = sent.copy()
        for m in range(n_frames):
            for c in range(I):
                rs_cases.ref.corrupt(rng, got[m], I, c, [0, code.t, 1, 2][(m + c) % 4])
        mk = np.array([(CCSDS_ASM[0] >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)
        frames = np.concatenate([np.broadcast_to(mk, (n_frames, 32)), np.unpackbits(got ^ pad, axis=1)], axis=1)
        rows.append(np.packbits(np.concatenate([rng.integers(0, 2, size=lead, dtype=np.uint8), frames.reshape(-1),
                                                rng.integers(0, 2, size=900 - lead, dtype=np.uint8)])))
        wants.append((sent, lead, crc_numpy(CCSDS_CRC16, sent, data_bits) ^ crc_field_numpy(CCSDS_CRC16, sent, data_bits)))
    n_bits = 900 + n_frames * P
    d_bytes = torch.from_numpy(rows[0]).cuda()
    d_pad = torch.from_numpy(pad).cuda()
    lock = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    cap = dec.frames_capacity(n_bits, P)
    out = (torch.empty((1, cap, code.n * I), dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
           torch.empty((1, cap), dtype=torch.int32, device="cuda"), torch.empty((1, (P + 6) // 8), dtype=torch.uint8, device="cuda"),
           torch.empty(1, dtype=torch.int32, device="cuda"))
    status = torch.empty((1, cap, I), dtype=torch.int32, device="cuda")
    crc, syn = (torch.empty((1, cap), dtype=torch.int32, device="cuda") for _ in range(2))

    def chain():
        dec.frames_extract(d_bytes, n_bits, P, 0, lock, marker=CCSDS_ASM[0], marker_bits=32, drop_bits=d, pad=d_pad, out=out)
        dec.rs_decode(code, out[0], out[1], I, status=status)
        dec.crc_check(CCSDS_CRC16, out[0], data_bits, 0, out[1], crc_out=crc, syndrome_out=syn)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for row, (sent, lead, want_syn) in zip(rows, wants):
        d_bytes.copy_(torch.from_numpy(row).cuda())
        lock.copy_(torch.tensor([[lead, 0, 0, 0]], dtype=torch.int32))
        crc.fill_(POISON32), syn.fill_(POISON32)
        graph.replay()
        torch.cuda.synchronize()
        assert int(out[1].item()) == n_frames and (status[0, :n_frames] >= 0).all().item()
        assert np.array_equal(out[0][0, :n_frames].cpu().numpy(), sent)
        assert np.array_equal(u32(syn)[0, :n_frames], want_syn) and (want_syn != 0).tolist() == [False, True, False, False]
        assert np.array_equal(u32(crc)[0, :n_frames], crc_numpy(CCSDS_CRC16, sent, data_bits))
        assert (crc[0, n_frames:] == POISON32).all().item() and (syn[0, n_frames:] == POISON32).all().item()


def test_pdcch_like_blocks_the_syndrome_is_the_rnti():
    """512 blocks of 27 payload bits + LTE_CRC16 XOR a per-block RNTI, tail-biting K = 7 R = 1/3, decoded and checked on the card"""
    import torch
    conv, pc, dec = decoder(3)
    assert (conv.K, conv.R) == (7, 3)
    F, L = 512, 43
    rng = np.random.default_rng(27)
    rnti = rng.integers(1, 1 << 16, size=F)
    payload = rng.integers(0, 256, size=(F, 4), dtype=np.uint8)
    payload[:, 3] &= 0xE0                                          # 27 bits
    sent = crc_append_numpy(LTE_CRC16, payload, 27, mask=rnti)
    assert sent.shape == (F, 6) and not (sent[:, 5] & 0x1F).any()
    sym = dec.encode(torch.from_numpy(sent).cuda(), L, tail=False, tail_biting=True)
    # noise-free: every syndrome is its RNTI
    out = dec.decode_tail_biting(sym, L)
    crc, syn = dec.crc_check(LTE_CRC16, out, 27)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), sent) and np.array_equal(u32(syn), rnti)
    assert np.array_equal(u32(crc), crc_numpy(LTE_CRC16, sent, 27))
    # with noise: the card's syndromes are those of the rule on the decoded bytes, and the RNTI exactly where the block came through
    mid = (pc.soft_decision_high + pc.soft_decision_low) / 2
    hard = (sym.cpu().numpy() > mid).astype(np.uint8)
    noisy = synth.quantise_numpy(hard, pc.soft_decision_high, pc.soft_decision_low, 0.0, conv.R, rng, pc.soft_dtype)
    out = dec.decode_tail_biting(torch.from_numpy(noisy).cuda(), L)
    crc, syn = dec.crc_check(LTE_CRC16, out, 27)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = crc_numpy(LTE_CRC16, got, 27) ^ crc_field_numpy(LTE_CRC16, got, 27)
    assert np.array_equal(u32(syn), want)
    came_through = (np.unpackbits(got, axis=1)[:, :L] == np.unpackbits(sent, axis=1)[:, :L]).all(axis=1)
    print("blocks decoded as sent:", int(came_through.sum()), "of", F)
    assert np.array_equal(u32(syn) == rnti, came_through)


def ccsds_streams(seed, I, n_frames, streams, flip):
    """CCSDS frames whose last two data bytes are the FECF; `flip` = (stream, frame): one data bit of that frame is flipped BEFORE the
    Reed-Solomon encoder -- a valid codeword that is not the frame that was checked.  A few byte errors behind the encoder in every
    codeword.  returns (symbols on the device [streams][steps][R], the frames as the RS encoder saw them, pad, P, data bits)"""
    import torch
    dec = decoder()[2]
    code = CCSDS_RS_255_223_DUAL
    rng = np.random.default_rng(seed)
    data_bits = 8 * (code.k * I - 2)
    payload = crc_append_numpy(CCSDS_CRC16, rng.integers(0, 256, size=(streams, n_frames, code.k * I - 2), dtype=np.uint8), data_bits)
    payload[flip[0], flip[1], 100] ^= 0x20
    sent = rs_encode_numpy(code, payload, I)
    got = sent.copy()
    for i in range(streams):
        for m in range(n_frames):
            for c in range(I):
                rs_cases.ref.corrupt(rng, got[i, m], I, c, (i + m + 3 * c) % (code.t + 1))
    P = 32 + 8 * code.n * I
    pad = frame_sync.ccsds_randomizer(code.n * I)
    mk = np.array([(CCSDS_ASM[0] >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)
    bits = np.concatenate([np.broadcast_to(mk, (streams, n_frames, 32)), np.unpackbits(got ^ pad, axis=2)], axis=2).reshape(streams, -1)
    d_sym = dec.encode(torch.from_numpy(np.packbits(bits, axis=1)).cuda(), bits.shape[1], tail=True)
    return d_sym, sent, pad, P, data_bits


def test_ccsds_chain_through_the_stream_decoder():
    """StreamDecoder with marker, frames, rs and frame_crc: syndrome 0 for every frame Reed-Solomon passed -- but for the one whose data
    bit was flipped in front of the encoder: rs_status >= 0, syndrome != 0.  The case Reed-Solomon cannot see"""
    conv, pc, dec = decoder()
    code, I, n_frames = CCSDS_RS_255_223_DUAL, 1, 8
    d_sym, sent, pad, P, data_bits = ccsds_streams(5, I, n_frames, 1, (0, 5))
    rx = StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=32, frame_pad=pad, rs=code)
    rx.frame_crc(CCSDS_CRC16, n_bits=data_bits)
    empty = rx.take_frames()
    assert len(empty) == 4 and empty[3].shape == (0,) and empty[3].dtype == np.int64
    cut = (3 * P + 111) * conv.R
    flat = d_sym[0].reshape(-1)
    rx.push(flat[:cut])
    first = rx.take_frames()
    rx.finish(flat[cut:])
    second = rx.take_frames()
    assert len(first) == len(second) == 4 and len(first[0]) >= 2 and len(second[0]) >= 2
    frames, errors, status, syndrome = (np.concatenate([a, b]) for a, b in zip(first, second))
    assert frames.shape == (n_frames, code.n * I) and syndrome.shape == (n_frames,) and syndrome.dtype == np.int64
    assert (status >= 0).all() and (status > 0).any() and np.array_equal(frames, sent[0])
    assert (syndrome != 0).tolist() == [m == 5 for m in range(n_frames)]
    assert np.array_equal(syndrome, crc_numpy(CCSDS_CRC16, frames, data_bits) ^ crc_field_numpy(CCSDS_CRC16, frames, data_bits))
    # without rs= the check runs behind the extraction, on the frames as received
    plain = StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=32, frame_pad=pad)
    plain.frame_crc(CCSDS_CRC16, n_bits=data_bits)
    plain.push(flat[:cut])
    plain.finish(flat[cut:])
    raw, _, raw_syndrome = plain.take_frames()
    assert np.array_equal(raw_syndrome, crc_numpy(CCSDS_CRC16, raw, data_bits) ^ crc_field_numpy(CCSDS_CRC16, raw, data_bits))
    assert len(raw) == n_frames and (raw_syndrome != 0).any()


def test_two_streams_through_the_multi_stream_decoder():
    conv, pc, dec = decoder()
    code, I, n_frames = CCSDS_RS_255_223_DUAL, 5, 3
    d_sym, sent, pad, P, data_bits = ccsds_streams(6, I, n_frames, 2, (1, 1))
    assert data_bits == 8904
    rx = MultiStreamDecoder(dec, 2, 1024, marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=32, frame_pad=pad, rs=code, rs_interleave=I)
    rx.frame_crc(CCSDS_CRC16, data_bits)
    taken = [[], []]
    cuts = [0, P * 2 + 500, P * 2 + 7000, d_sym.shape[1]]
    for a, b in zip(cuts[:-1], cuts[1:]):
        rx.push(d_sym[:, a:b]) if b < d_sym.shape[1] else rx.finish(d_sym[:, a:b])
        for i, t4 in enumerate(rx.take_frames()):
            assert len(t4) == 4 and len(t4[0]) == len(t4[1]) == len(t4[2]) == len(t4[3])
            taken[i].append(t4)
    assert sum(len(t4[0]) > 0 for t4 in taken[0]) >= 2
    for i in range(2):
        frames, errors, status, syndrome = (np.concatenate([t4[k] for t4 in taken[i]]) for k in range(4))
        assert (status >= 0).all() and status.shape == (n_frames, I) and np.array_equal(frames, sent[i])
        assert (syndrome != 0).tolist() == [(i, m) == (1, 1) for m in range(n_frames)]


def test_frame_crc_rejections():
    conv, pc, dec = decoder()
    code, I = CCSDS_RS_255_223_DUAL, 1
    P = 32 + 8 * code.n
    pad = frame_sync.ccsds_randomizer(code.n)
    kw = dict(marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=32, frame_pad=pad, rs=code)
    with pytest.raises(ValueError, match="frames=True"):
        StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P).frame_crc(CCSDS_CRC16, 8)
    with pytest.raises(ValueError, match="exceeds"):
        StreamDecoder(dec, 1024, **kw).frame_crc(CCSDS_CRC16, 8 * code.n - 15)
    with pytest.raises(ValueError, match="exceeds"):
        StreamDecoder(dec, 1024, **kw).frame_crc(CCSDS_CRC16, 8 * code.n - 16, first_bit=1)
    StreamDecoder(dec, 1024, **kw).frame_crc(CCSDS_CRC16, 8 * code.n - 16)                  # the field may end the frame
    for more in (dict(deinterleave=(12, 17)), dict(deinterleave=(12, 17), dvb_derandomize=True)):
        dvb = MultiStreamDecoder(dec, 2, 1024, marker=(0x47, 8), period=8 * 204, frames=True, **more)
        with pytest.raises(ValueError, match="transport packets"):
            dvb.frame_crc(CCSDS_CRC16, 64)
    rx = StreamDecoder(dec, 1024, **kw)
    d_sym, _, _, _, data_bits = ccsds_streams(5, I, 2, 1, (0, 0))
    rx.push(d_sym[0].reshape(-1)[:64])
    with pytest.raises(ValueError, match="before the first push"):
        rx.frame_crc(CCSDS_CRC16, data_bits)
    assert len(rx.take_frames()) == 3                                                       # and nothing changed
