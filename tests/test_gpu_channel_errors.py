"""vit_hip_encode_batch and vit_hip_channel_errors_batch on the device: the encoder against the oracle's (which
tests/test_channel_errors_cpu.py pins to the reference's two encoders) and against the frame generator's noise-free branch; the
state numbering against the decoder's start / end states; the counts against the numpy mirror of the counting rule, on noisy
frames, on planted flips, through depuncturing, with frame strides, and on the three reduction shapes (one long frame, many
short frames, a workgroup that sums several chunks per thread); overwrite semantics, graph capture, argument errors; and the running
totals of StreamDecoder / MultiStreamDecoder."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, BatchDecoder, MultiStreamDecoder, StreamDecoder, ViterbiBranchTable, ViterbiDecoder_Config,
                                   _lib, get_decoding_config, synth)
from tests.helpers import DECODE_TYPES, default_ebn0, make_table_config

pytestmark = pytest.mark.gpu

VOYAGER, LTE, DAB, IS95, CASSINI = 2, 3, 4, 5, 7


@functools.lru_cache(maxsize=None)
def decoder(code_id, decode_type):
    code = COMMON_CODES[code_id]
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config)


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mask_pad(data, L):
    """the bytes with the pad bits of the last byte cleared"""
    out = data.copy()
    if L % 8:
        out[:, -1] &= np.uint8((0xFF << (8 - L % 8)) & 0xFF)
    return out


def random_bytes(rng, F, L):
    """[F][ceil(L/8)] random bytes, the pad bits random too: they are not data"""
    return rng.integers(0, 256, size=(F, (L + 7) // 8), dtype=np.uint8)


def coded_terminated(code, data, L):
    """re-encoded bits [F][L + K-1][R] of terminated frames: with the pad bits cleared, the first L + K-1 steps of the whole-byte
    encoder (zero tail) are the frame's"""
    return synth.encode_bits_numpy(code.K, code.R, code.G, mask_pad(data, L))[:, :L + code.K - 1]


def levels(pc, coded):
    return np.where(coded != 0, pc.soft_decision_high, pc.soft_decision_low).astype(pc.soft_dtype)


def flip(pc, sym, positions):
    """sym [F][S][R] with the symbols at the flat (frame, index) positions inverted (high <-> low)"""
    flat = sym.reshape(sym.shape[0], -1)
    for f, k in positions:
        flat[f, k] = pc.soft_decision_high + pc.soft_decision_low - flat[f, k]
    return sym


def disturb(pc, sym, rng, p_flip=0.04, p_erase=0.02):
    """noise-free symbols with a share inverted and a share moved to the midpoint"""
    r = rng.random(sym.shape)
    out = np.where(r < p_flip, pc.soft_decision_high + pc.soft_decision_low - sym, sym)
    return np.where(r > 1.0 - p_erase, (pc.soft_decision_high + pc.soft_decision_low) // 2, out).astype(pc.soft_dtype)


def counts(got):
    return got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy().astype(np.int64)


# ---- encoder -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("decode_type", DECODE_TYPES)
@pytest.mark.parametrize("code_id", range(len(COMMON_CODES)))
def test_encode_terminated_frames(oracle, code_id, decode_type):
    import torch
    code, pc, dec = decoder(code_id, decode_type)
    F = 130
    for L in (code.K, 41, 1000):
        rng = np.random.default_rng(1000 * code_id + L)
        data = random_bytes(rng, F, L)
        sym, end = dec.encode(cuda(data), L, end_state_out=True)
        n = (L + code.K - 1) * code.R
        want = np.stack([oracle.encode(code.K, code.R, code.G, row)[:n] for row in mask_pad(data, L)]).reshape(F, -1, code.R)
        assert sym.shape == (F, L + code.K - 1, code.R)
        assert np.array_equal(sym.cpu().numpy(), levels(pc, want)), (code.name, L)
        assert not end.cpu().numpy().any(), "a terminated frame ends in state 0"
        if L % 8 == 0:
            tx, ssym = dec.synth(F, L, None, seed=L)                        # the generator's noise-free branch on its own bytes
            assert torch.equal(dec.encode(tx, L), ssym), (code.name, L)


def test_encode_three_bytes_of_history(oracle):
    code, pc, dec = decoder(CASSINI, "SOFT16")
    F, L = 3, 41
    data = random_bytes(np.random.default_rng(5), F, L)
    want = np.stack([oracle.encode(code.K, code.R, code.G, row)[:(L + 14) * 6] for row in mask_pad(data, L)]).reshape(F, -1, 6)
    assert np.array_equal(dec.encode(cuda(data), L).cpu().numpy(), levels(pc, want))


@pytest.mark.parametrize("decode_type", ["SOFT16", "HARD8"])
@pytest.mark.parametrize("L", [7, 40, 41])
def test_encode_tail_biting_frames(L, decode_type):
    code, pc, dec = decoder(LTE, decode_type)
    F = 4099
    rng = np.random.default_rng(L)
    data = random_bytes(rng, F, L)
    bits = np.unpackbits(data, axis=1)[:, :L]
    sym, end = dec.encode(cuda(data), L, tail_biting=True, end_state_out=True)
    assert np.array_equal(sym.cpu().numpy(), levels(pc, synth.encode_tail_biting_numpy(code.K, code.R, code.G, bits)))
    want_end = sum(bits[:, L - 1 - j].astype(np.int64) << j for j in range(code.K - 1))     # ends where it started
    assert np.array_equal(end.cpu().numpy(), want_end)


def test_encode_continued_in_pieces():
    """one terminated frame re-encoded as five unequal pieces, each from the end state of the one before and re-packed from its own
    bit 0: cuts at 1000 (a byte boundary), 1003 and 3500 (inside a byte), 2048"""
    import torch
    code, pc, dec = decoder(VOYAGER, "SOFT16")
    L = 4096
    data = random_bytes(np.random.default_rng(9), 1, L)
    bits = np.unpackbits(data, axis=1)[0]
    whole = dec.encode(cuda(data), L)
    cuts = [0, 1000, 1003, 2048, 3500, L]
    state, pieces = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        piece = cuda(np.packbits(bits[a:b])[None, :])
        last = b == L
        sym, state = dec.encode(piece, b - a, tail=last, start_state=state, end_state_out=True)
        assert sym.shape[1] == b - a + (code.K - 1 if last else 0)
        want_state = 0 if last else sum(int(bits[b - 1 - j]) << j for j in range(code.K - 1))
        assert int(state.item()) == want_state
        pieces.append(sym)
    assert torch.equal(torch.cat(pieces, dim=1), whole)


@pytest.mark.parametrize("code_id", [0, VOYAGER, IS95])
def test_state_numbering_is_the_decoders(code_id):
    """noise-free symbols of an unterminated piece from random non-zero start states, decoded by update(start_state) and
    chainback(end_state = the encoder's end state), give back the info bits"""
    code, pc, dec = decoder(code_id, "SOFT16")
    F, steps = 37, 203
    rng = np.random.default_rng(code_id)
    data = random_bytes(rng, F, steps)
    start = rng.integers(1, 1 << (code.K - 1), size=F)
    sym, end = dec.encode(cuda(data), steps, tail=False, start_state=start, end_state_out=True)
    Lp = steps - (code.K - 1)
    dec.update(sym, Lp, n_steps=steps, start_state=start, want_metrics=False)
    out = dec.chainback(F, Lp, end_state=end).cpu().numpy()
    assert np.array_equal(np.unpackbits(out, axis=1)[:, :Lp], np.unpackbits(data, axis=1)[:, :Lp])
    assert end.cpu().numpy().any()


# ---- counts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("decode_type", DECODE_TYPES)
@pytest.mark.parametrize("code_id", [VOYAGER, LTE, DAB, IS95])
def test_counts_of_noisy_decoded_frames(code_id, decode_type):
    code, pc, dec = decoder(code_id, decode_type)
    F = 130
    for L in (1000, 41):
        rng = np.random.default_rng(code_id * 100 + L)
        data = mask_pad(random_bytes(rng, F, L), L)
        sym = synth.quantise_numpy(coded_terminated(code, data, L), pc.soft_decision_high, pc.soft_decision_low,
                                   default_ebn0(code, decode_type), code.R, rng, pc.soft_dtype)
        d_sym = cuda(sym)
        out = dec.decode(d_sym, L)
        err, cmp = counts(dec.channel_errors(d_sym, out, L))
        want = synth.channel_errors_numpy(code, pc.soft_decision_high, pc.soft_decision_low, sym, coded_terminated(code, out.cpu().numpy(), L))
        assert np.array_equal(err, want[0]) and np.array_equal(cmp, want[1]), (code.name, decode_type, L)
        assert err.sum() > 0 and (decode_type == "HARD8" or (cmp < sym[0].size).any())      # errors and midpoint symbols occur


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_counts_of_planted_flips(decode_type):
    code, pc, dec = decoder(VOYAGER, decode_type)
    F, L, R = 5, 1000, code.R
    S = L + code.K - 1
    data = random_bytes(np.random.default_rng(3), F, L)
    planted = [(0, 0), (0, (L - 1) * R), (0, S * R - 1), (0, 8 * R - 1), (0, 8 * R),         # step 0, last info step, last tail step, a thread boundary
               (1, S * R - 1), (2, 0), (4, 8 * R - 1)]                                       # last symbol of a frame, first of the next
    sym = flip(pc, levels(pc, coded_terminated(code, data, L)), planted)
    err, cmp = counts(dec.channel_errors(cuda(sym), cuda(data), L))
    assert err.tolist() == [5, 1, 1, 0, 1] and cmp.tolist() == [S * R] * F


@pytest.mark.parametrize("decode_type", ["SOFT16", "HARD8"])
def test_counts_skip_what_depuncturing_inserted(decode_type):
    from tests.test_gpu_punctured import TOTAL_DATA_BITS, puncture_mask
    code, pc, dec = decoder(DAB, decode_type)
    F, L, R = 5, TOTAL_DATA_BITS, code.R
    S = L + code.K - 1
    mask = puncture_mask()
    data = random_bytes(np.random.default_rng(4), F, L)
    planted = [(0, 0), (0, 3), (0, (L - 1) * R), (0, S * R - 1), (0, S * R - 4), (0, 8 * R - 1), (0, 8 * R), (1, S * R - 1), (1, S * R - 3),
               (2, 0), (2, 1), (4, 8 * R - 2)]
    sym = flip(pc, levels(pc, coded_terminated(code, data, L)), planted).reshape(F, -1)
    d_sym = dec.depuncture(cuda(sym[:, mask]), mask)
    err, cmp = counts(dec.channel_errors(d_sym, cuda(data), L))
    survive = [sum(1 for f, k in planted if f == g and mask[k]) for g in range(F)]
    assert 0 < sum(survive) < len(planted)
    assert err.tolist() == survive and cmp.tolist() == [int(mask.sum())] * F


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_frame_strides(decode_type):
    """symbol stride steps*R + 3 (every other frame misaligned for the vector loads / stores), byte stride ceil(L/8) + 5"""
    import torch
    code, pc, dec = decoder(VOYAGER, decode_type)
    F, L = 9, 1000
    n, nb = (L + code.K - 1) * code.R, (L + 7) // 8
    rng = np.random.default_rng(6)
    data = random_bytes(rng, F, L)
    sym = disturb(pc, levels(pc, coded_terminated(code, data, L)), rng)
    packed = counts(dec.channel_errors(cuda(sym), cuda(data), L))
    assert packed[0].min() > 0
    wide_sym = np.full((F, n + 3), 0x5A, dtype=pc.soft_dtype)
    wide_sym[:, :n] = sym.reshape(F, -1)
    wide_data = np.full((F, nb + 5), 0xC3, dtype=np.uint8)
    wide_data[:, :nb] = data
    d_wide_sym, d_wide_data = cuda(wide_sym), cuda(wide_data)
    strided = counts(dec.channel_errors(d_wide_sym, d_wide_data, L))
    assert np.array_equal(strided[0], packed[0]) and np.array_equal(strided[1], packed[1])
    flat = counts(dec.channel_errors(d_wide_sym.reshape(-1), d_wide_data.reshape(-1)[:(F - 1) * (nb + 5) + nb], L,
                                     symbol_frame_stride=n + 3, bytes_frame_stride=nb + 5))
    assert np.array_equal(flat[0], packed[0]) and np.array_equal(flat[1], packed[1])
    # encode into the strided buffer: the guard words between the frames stay
    out = torch.full((F, n + 3), 0x5A, dtype=d_wide_sym.dtype, device="cuda")
    assert dec.encode(d_wide_data, L, out=out) is out
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :n], dec.encode(cuda(data), L).cpu().numpy().reshape(F, -1))
    assert (got[:, n:] == 0x5A).all()


@pytest.mark.parametrize("F,L", [(1, 100003), (1, 8 * 16384 + 5), (2, 8 * 16384 + 5)])
def test_reduction_of_long_frames(F, L):
    """one frame over many workgroups; from 16384 chunks per frame on a workgroup sums 8 chunks per thread (the last workgroup of a
    frame is partial; with two frames one workgroup spans both)"""
    code, pc, dec = decoder(VOYAGER, "SOFT16")
    rng = np.random.default_rng(L + F)
    data = random_bytes(rng, F, L)
    coded = coded_terminated(code, data, L)
    sym = disturb(pc, levels(pc, coded), rng)
    err, cmp = counts(dec.channel_errors(cuda(sym), cuda(data), L))
    want = synth.channel_errors_numpy(code, pc.soft_decision_high, pc.soft_decision_low, sym, coded)
    assert np.array_equal(err, want[0]) and np.array_equal(cmp, want[1])
    assert err.min() > 1000 and (cmp < sym[0].size).all()


@pytest.mark.parametrize("decode_type", ["SOFT16", "HARD8"])
def test_reduction_of_short_tail_biting_frames(decode_type):
    """4099 frames of 40 steps at R = 3: five chunks per frame, a wave spans thirteen frames"""
    code, pc, dec = decoder(LTE, decode_type)
    F, L = 4099, 40
    rng = np.random.default_rng(8)
    data = random_bytes(rng, F, L)
    coded = synth.encode_tail_biting_numpy(code.K, code.R, code.G, np.unpackbits(data, axis=1)[:, :L])
    sym = disturb(pc, levels(pc, coded), rng)
    err, cmp = counts(dec.channel_errors(cuda(sym), cuda(data), L, tail_biting=True))
    want = synth.channel_errors_numpy(code, pc.soft_decision_high, pc.soft_decision_low, sym, coded)
    assert np.array_equal(err, want[0]) and np.array_equal(cmp, want[1])
    assert err.sum() > F and len(set(err.tolist())) > 3


def raw_counts(dec, d_sym, d_bytes, F, L, flags, d_err, d_cmp, start=None, sym_stride=0, byte_stride=0):
    return _lib.load().vit_hip_channel_errors_batch(
        dec._handle._h, C.c_void_p(d_sym.data_ptr()) if d_sym is not None else None, sym_stride,
        C.c_void_p(d_bytes.data_ptr()) if d_bytes is not None else None, byte_stride, F, L, flags,
        C.c_void_p(start.data_ptr()) if start is not None else None, C.c_void_p(d_err.data_ptr()) if d_err is not None else None,
        C.c_void_p(d_cmp.data_ptr()) if d_cmp is not None else None, dec._stream())


def raw_encode(dec, d_bytes, F, L, flags, d_out, start=None, d_end=None, sym_stride=0, byte_stride=0):
    return _lib.load().vit_hip_encode_batch(
        dec._handle._h, C.c_void_p(d_bytes.data_ptr()) if d_bytes is not None else None, byte_stride, F, L, flags,
        C.c_void_p(start.data_ptr()) if start is not None else None, C.c_void_p(d_out.data_ptr()) if d_out is not None else None,
        sym_stride, C.c_void_p(d_end.data_ptr()) if d_end is not None else None, dec._stream())


def test_counts_are_overwritten_and_the_call_captures_into_a_graph():
    import torch
    code, pc, dec = decoder(VOYAGER, "SOFT16")
    F, L = 70, 1000
    rng = np.random.default_rng(12)
    data = random_bytes(rng, F, L)
    coded = coded_terminated(code, data, L)
    sym = disturb(pc, levels(pc, coded), rng)
    want = synth.channel_errors_numpy(code, pc.soft_decision_high, pc.soft_decision_low, sym, coded)
    d_sym, d_data = cuda(sym), cuda(data)
    d_err = torch.full((F,), -1, dtype=torch.int32, device="cuda")          # 0xFFFFFFFF
    d_cmp = torch.full((F,), -1, dtype=torch.int32, device="cuda")
    for _ in range(2):
        assert raw_counts(dec, d_sym, d_data, F, L, _lib.ENCODE_TAIL, d_err, d_cmp) == _lib.OK
        assert np.array_equal(d_err.cpu().numpy(), want[0]) and np.array_equal(d_cmp.cpu().numpy(), want[1])
    # d_compared is optional
    d_err.fill_(-1)
    assert raw_counts(dec, d_sym, d_data, F, L, _lib.ENCODE_TAIL, d_err, None) == _lib.OK
    assert np.array_equal(d_err.cpu().numpy(), want[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert raw_counts(dec, d_sym, d_data, F, L, _lib.ENCODE_TAIL, d_err, d_cmp) == _lib.OK
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_err.cpu().numpy(), want[0]) and np.array_equal(d_cmp.cpu().numpy(), want[1])


def test_argument_errors_launch_nothing():
    """return codes only: every rejected call leaves the sentinel in its outputs"""
    import torch
    code, pc, dec = decoder(VOYAGER, "SOFT16")
    K, R = code.K, code.R
    F, L = 3, 64
    n, nb = (L + K - 1) * R, L // 8
    d_sym = torch.full((F * n + 64,), 77, dtype=torch.int16, device="cuda")
    d_data = torch.zeros(F * nb + 64, dtype=torch.uint8, device="cuda")
    d_err = torch.full((F,), 0x1234, dtype=torch.int32, device="cuda")
    d_cmp = torch.full((F,), 0x1234, dtype=torch.int32, device="cuda")
    d_end = torch.full((F,), 0x1234, dtype=torch.int32, device="cuda")
    d_start = torch.zeros(F, dtype=torch.int32, device="cuda")
    T, TB, BAD = _lib.ENCODE_TAIL, _lib.ENCODE_TAIL_BITING, _lib.ERR_INVALID_ARG
    bad_counts = [
        dict(d_sym=None), dict(d_bytes=None), dict(d_err=None), dict(L=0), dict(flags=T | TB), dict(flags=4), dict(flags=T | 8),
        dict(flags=TB, L=K - 1), dict(flags=TB, start=d_start), dict(sym_stride=n - 1), dict(byte_stride=nb - 1),
        dict(F=1, L=(1 << 32) // R), dict(F=1, L=(1 << 32) // R - (K - 1)),
    ]
    for kw in bad_counts:
        a = dict(dec=dec, d_sym=d_sym, d_bytes=d_data, F=F, L=L, flags=T, d_err=d_err, d_cmp=d_cmp)
        a.update(kw)
        assert raw_counts(**a) == BAD, kw
    bad_encode = [
        dict(d_bytes=None), dict(d_out=None), dict(L=0), dict(flags=T | TB), dict(flags=4), dict(flags=TB, L=K - 1),
        dict(flags=TB, start=d_start), dict(sym_stride=n - 1), dict(byte_stride=nb - 1), dict(F=1, L=(1 << 32) // R - (K - 1)),
    ]
    for kw in bad_encode:
        a = dict(dec=dec, d_bytes=d_data, F=F, L=L, flags=T, d_out=d_sym, d_end=d_end)
        a.update(kw)
        assert raw_encode(**a) == BAD, kw
    # frames = 0 is no work and no error
    assert raw_counts(dec, d_sym, d_data, 0, L, T, d_err, d_cmp) == _lib.OK
    assert raw_encode(dec, d_data, 0, L, T, d_sym, d_end=d_end) == _lib.OK
    # a two-valued table that is no convolutional code's
    table = ViterbiBranchTable(K, R, code.G, pc.soft_decision_high, pc.soft_decision_low, pc.soft_dtype)
    table._table[0, 5] = pc.soft_decision_high + pc.soft_decision_low - table._table[0, 5]
    odd = BatchDecoder(table, ViterbiDecoder_Config.from_decoder_config(pc))
    assert odd._handle.info.table_is_linear == 0
    assert raw_counts(odd, d_sym, d_data, F, L, T, d_err, d_cmp) == _lib.ERR_UNSUPPORTED
    assert raw_encode(odd, d_data, F, L, T, d_sym, d_end=d_end) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (d_sym == 77).all() and (d_err == 0x1234).all() and (d_cmp == 0x1234).all() and (d_end == 0x1234).all()


# ---- streams -----------------------------------------------------------------------------------------------------------------

W, HEAD, TAIL, T_STREAM = 128, 48, 48, 5000


def stream_symbols(pc, code, seed, flips):
    """a noise-free terminated stream of T_STREAM steps [T][R] with the symbols of `flips` (flat indices) inverted"""
    L = T_STREAM - (code.K - 1)
    data = mask_pad(random_bytes(np.random.default_rng(seed), 1, L), L)
    sym = flip(pc, levels(pc, coded_terminated(code, data, L)), [(0, k) for k in flips])
    return data[0], sym[0]


# steps 138 (the head of window 1 and the body of window 0), 175 / 176 (the edge between what windows 0 and 1 emit), 3900 (the tail of
# one window, the body of the next), and two of the final K-1 tail steps
FLIPS = [2 * 50, 2 * 138 + 1, 2 * 175, 2 * 176 + 1, 2 * 1000, 2 * 2500 + 1, 2 * 3900, 2 * 4995, 2 * 4999 + 1]


def test_stream_decoder_keeps_running_totals():
    code, pc, dec = decoder(VOYAGER, "SOFT16")
    data, sym = stream_symbols(pc, code, 21, FLIPS)
    d_sym = cuda(sym)
    nb = (T_STREAM - (code.K - 1) + 7) // 8
    calls = {}
    for size in (700, T_STREAM):
        sd = StreamDecoder(dec, W, HEAD, TAIL, channel_errors=True)
        got = b"".join(sd.push(d_sym[k:k + size]) for k in range(0, T_STREAM, size)) + sd.finish()
        assert np.array_equal(np.frombuffer(got, dtype=np.uint8), data[:nb])             # nine isolated flips are corrected
        assert sd.channel_errors == (9, T_STREAM * 2), size
        calls[size] = sd.calls
    assert len(calls[700]) > 2 and len(calls[T_STREAM]) == 2
    plain = StreamDecoder(dec, W, HEAD, TAIL)
    got = b"".join(plain.push(d_sym[k:k + 700]) for k in range(0, T_STREAM, 700)) + plain.finish()
    direct, n_bits = dec.decode_stream(d_sym, True, True, W, HEAD, TAIL)
    assert n_bits == T_STREAM - (code.K - 1) and got == direct.cpu().numpy().tobytes()
    assert not hasattr(plain, "channel_errors") and plain.calls == calls[700]           # the same internal calls, nothing added


def test_multi_stream_decoder_keeps_totals_per_stream():
    import torch
    code, pc, dec = decoder(VOYAGER, "SOFT16")
    flips = [FLIPS[:2], [], FLIPS[2:7] + FLIPS[8:]]
    made = [stream_symbols(pc, code, 30 + s, flips[s]) for s in range(3)]
    d_sym = torch.stack([cuda(sym) for _, sym in made])
    for count in (True, False):
        md = MultiStreamDecoder(dec, 3, W, HEAD, TAIL, channel_errors=count)
        parts = [md.push(d_sym[:, k:k + 700]) for k in range(0, T_STREAM, 700)] + [md.finish()]
        for s in range(3):
            direct, _ = dec.decode_stream(d_sym[s].contiguous(), True, True, W, HEAD, TAIL)
            assert b"".join(p[s] for p in parts) == direct.cpu().numpy().tobytes(), (count, s)
        if count:
            assert md.channel_errors[0].tolist() == [2, 0, 6] and md.channel_errors[1].tolist() == [T_STREAM * 2] * 3
        else:
            assert not hasattr(md, "channel_errors")
