"""BatchDecoder.rs_decode / vit_hip_rs_decode_batch on the GPU against tests/rs_reference.py (never the code under test): whole output
buffers, written or not, and every status entry -- all stock codes in both bases, the nroots = 2, 3 and 64 codes and a shortened one,
interleave depths 1, 2, 5, 8 and 11, batches 1x1, 3x2 and 2x5, 0 to 200 errors per codeword mixed inside a frame, a burst, the
all-zero and all-0xFF words; in place and out of place, strides with guard bytes, frame counts of 0, a part and above max_frames;
rejected arguments; a second pass over what those never reach -- all 16 primitive polynomials, nroots just above every power of two,
k = 1 codes, every error count 0 .. t + 2, words whose first or last syndromes vanish, roots in the virtual fill, miscorrection at t = 2
and 3, depths 9 .. 64 in several frames, frames of 3 bytes, the dword staging at every start, 70 000 blocks; frames_extract and rs_decode captured into one graph; the whole chain through StreamDecoder at 3 dB; and two streams at
depth 5 through MultiStreamDecoder."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (CCSDS_ASM, CCSDS_RS_255_223_DUAL, COMMON_CODES, BatchDecoder, MultiStreamDecoder, StreamDecoder, _lib, frame_sync,
                                   rs_decode_numpy, rs_encode_numpy, synth)
from tests import frames_reference as fr
from tests import rs_cases
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON32 = np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0]


@functools.lru_cache(maxsize=None)
def decoder():
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, "SOFT16")
    return code, pc, BatchDecoder(table, config)


def ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def run(case, in_place, extra=0, counts=None, lead=0):
    """the case's frames in a poisoned buffer `lead` bytes into an allocation, frames n I + extra bytes apart -> (out buffer, status,
    expected out buffer, expected status), all numpy"""
    import torch
    dec = decoder()[2]
    code, I, rows, mf = case["code"], case["I"], case["rows"], case["max_frames"]
    nI = code.n * I
    host = np.full((rows, mf, nI + extra), POISON, dtype=np.uint8)
    host[..., :nI] = case["got"]
    raw = torch.full((lead + host.size,), POISON, dtype=torch.uint8, device="cuda")
    d_in = raw[lead:].view(rows, mf, nI + extra)
    d_in.copy_(torch.from_numpy(host).cuda())
    d_out = None if in_place else torch.full_like(d_in, POISON)
    d_status = torch.full((rows, mf, I), int(POISON32), dtype=torch.int32, device="cuda")
    d_n = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    got, status = dec.rs_decode(code, d_in[..., :nI] if extra else d_in, d_n, I, out=None if in_place else (d_out[..., :nI] if extra else d_out),
                                status=d_status)
    torch.cuda.synchronize()
    assert status is d_status
    want = host.copy() if in_place else np.full_like(host, POISON)
    want_status = np.full((rows, mf, I), POISON32, dtype=np.int32)
    for r in range(rows):
        live = mf if counts is None else min(counts[r], mf)
        want[r, :live, :nI] = case["want"][r, :live]
        want_status[r, :live] = case["status"][r, :live]
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy(), host)                        # the input is only read
    return (d_in if in_place else d_out).cpu().numpy(), d_status.cpu().numpy(), want, want_status


@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("shape", rs_cases.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_every_code_depth_batch_and_error_count(shape, in_place):
    case = rs_cases.make_case(*shape)
    got, status, want, want_status = run(case, in_place)
    assert np.array_equal(status, want_status), (status.reshape(-1).tolist(), want_status.reshape(-1).tolist())
    assert np.array_equal(got, want)


@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("shape,extra,lead", [(("ccsds223dual", 5, 2, 5), 7, 1), (("dvb", 5, 3, 2), 1, 3), (("nroots2", 1, 3, 2), 64, 2),
                                             (("ccsds239", 8, 3, 2), 4, 0)], ids=["223", "dvb", "nroots2", "239"])
def test_strides_with_guard_bytes_and_odd_alignments(shape, extra, lead, in_place):
    got, status, want, want_status = run(rs_cases.make_case(*shape), in_place, extra, None, lead)
    assert np.array_equal(status, want_status) and np.array_equal(got, want)


@pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("shape,counts", [(("dvb", 5, 3, 2), [0, 1, 7]), (("ccsds223dual", 5, 2, 5), [3, 0]), (("nroots2", 1, 3, 2), [2, 1, 0])],
                         ids=["dvb", "223", "nroots2"])
def test_frames_at_or_past_the_count_and_their_status_are_not_written(shape, counts, in_place):
    got, status, want, want_status = run(rs_cases.make_case(*shape), in_place, 3, counts)
    assert np.array_equal(status, want_status) and np.array_equal(got, want)
    assert (status == POISON32).any()


# ---- the second pass: the cases of tests/rs_cases.py below SHAPES (tests/test_rs_cpu.py checks what each of them holds) -------------

def equal(case, in_place, extra=0, counts=None, lead=0):
    got, status, want, want_status = run(case, in_place, extra, counts, lead)
    where = (case["I"], extra, counts, lead)
    assert np.array_equal(status, want_status), (where, np.argwhere(status != want_status)[:8].tolist())
    assert np.array_equal(got, want), (where, np.argwhere(got != want)[:8].tolist())
    return status


IN_PLACE = pytest.mark.parametrize("in_place", [True, False], ids=["inplace", "outofplace"])


@IN_PLACE
@pytest.mark.parametrize("name", rs_cases.SWEEPS)
def test_every_error_count_from_none_to_two_beyond_t(name, in_place):
    equal(rs_cases.make_sweep(name), in_place)


@IN_PLACE
@pytest.mark.parametrize("name,kinds", rs_cases.DESIGNED, ids=[d[0] for d in rs_cases.DESIGNED])
def test_vanishing_syndromes_in_front_and_behind_and_roots_in_the_fill(name, kinds, in_place):
    equal(rs_cases.make_designed(name, kinds), in_place)


@IN_PLACE
@pytest.mark.parametrize("name", rs_cases.MISCORRECTING)
def test_words_beyond_t_move_to_the_codeword_within_t_where_there_is_one(name, in_place):
    status = equal(rs_cases.make_miscorrecting(name), in_place)
    assert (status >= 0).sum() >= 20 and (status == -1).sum() >= 20


@IN_PLACE
@pytest.mark.parametrize("shape", rs_cases.GEOMETRY, ids=lambda s: "-".join(map(str, s)))
def test_every_polynomial_and_syndrome_geometry(shape, in_place):
    equal(rs_cases.make_case(*shape), in_place)


@IN_PLACE
@pytest.mark.parametrize("shape", rs_cases.TILED, ids=lambda s: "-".join(map(str, s)))
def test_several_tiles_and_several_frames(shape, in_place):
    """interleave depths 9, 11, 16, 17 and 64: plain, strides with guard bytes at every misalignment, and frame counts"""
    case = rs_cases.make_tiled(*shape)
    equal(case, in_place)
    for extra in (1, 7):
        for lead in (1, 2, 3):
            equal(case, in_place, extra, None, lead)
    for counts in ([[0, 1, 7]] if case["rows"] == 3 else [[2, 0], [1, 5]]):
        status = equal(case, in_place, 3, counts)
        assert (status == POISON32).any() and (status != POISON32).any()


@IN_PLACE
@pytest.mark.parametrize("shape", rs_cases.TINY, ids=lambda s: "-".join(map(str, s)))
def test_frames_shorter_than_the_way_to_the_next_dword(shape, in_place):
    """3, 6 and 9 bytes a frame, starting at every residue of 4"""
    case = rs_cases.make_case(*shape)
    for extra in (0, 1, 2):
        for lead in (0, 1, 2, 3):
            equal(case, in_place, extra, None, lead)
    equal(case, in_place, 1, [1, 0, 2], 3)


@IN_PLACE
@pytest.mark.parametrize("shape", rs_cases.DWORDS, ids=lambda s: "-".join(map(str, s)))
def test_the_dword_staging_at_every_start_and_end(shape, in_place):
    case = rs_cases.make_case(*shape)
    for extra in (1, 2, 3):
        for lead in (1, 2, 3):
            equal(case, in_place, extra, None, lead)


@IN_PLACE
def test_seventy_thousand_blocks(in_place):
    case = rs_cases.make_many()
    assert case["rows"] * case["max_frames"] == 70000 and case["got"].size == 210000
    equal(case, in_place)


def test_rejections_launch_nothing():
    import torch
    L, dec = _lib.load(), decoder()[2]
    case = rs_cases.make_case("dvb", 5, 3, 2)
    code, I, rows, mf = case["code"], 5, 3, 2
    nI = code.n * I
    buf = torch.full((2 * rows * mf * nI,), POISON, dtype=torch.uint8, device="cuda")
    status = torch.full((rows * mf * I,), int(POISON32), dtype=torch.int32, device="cuda")
    h, c = dec._handle._h, dec._rs_code(code)._c
    a, b = buf.data_ptr(), buf.data_ptr() + rows * mf * nI
    st = C.c_void_p(status.data_ptr())
    calls = [(None, c, a, a, 0, I, st), (h, None, a, a, 0, I, st), (h, c, None, a, 0, I, st), (h, c, a, None, 0, I, st), (h, c, a, a, 0, I, None),
             (h, c, a, a, 0, 0, st), (h, c, a, a, nI - 1, I, st), (h, c, a, a + 1, 0, I, st), (h, c, a + nI, a, 0, I, st),
             (h, c, a, b - 1, 0, I, st)]
    for hh, cc, src, dst, stride, depth, stat in calls:
        rc = L.vit_hip_rs_decode_batch(hh, cc, src, dst, stride, rows, mf, None, depth, stat, None)
        assert rc == _lib.ERR_INVALID_ARG, (src, dst, stride, depth)
    assert L.vit_hip_rs_decode_batch(h, c, a, b, 0, 0, mf, None, I, st, None) == _lib.OK
    torch.cuda.synchronize()
    assert (buf == POISON).all().item() and (status == int(POISON32)).all().item()
    for bad in (dict(gfpoly=0x11B), dict(gfpoly=0x87), dict(nroots=1), dict(nroots=65), dict(pad=223), dict(prim=3), dict(prim=0), dict(fcr=255),
                dict(dual_basis=2), dict(gfpoly=0x11D, dual_basis=1)):
        p = _lib.VitHipRsParams(**{**dict(gfpoly=0x187, fcr=112, prim=11, nroots=32, pad=0, dual_basis=0), **bad})
        out = C.c_void_p(1)
        assert L.vit_hip_rs_create(h, C.byref(p), C.byref(out)) == _lib.ERR_INVALID_ARG and not out.value, bad
    with pytest.raises(ValueError):
        dec.rs_decode(code, buf.view(rows, mf, 2 * nI)[..., :nI - 1], None, I)


def test_frames_extract_then_rs_decode_captured_into_a_graph():
    """one chain: the extraction writes the frames and their count, the decode reads both; replayed twice on changed input"""
    import torch
    dec = decoder()[2]
    code, I = rs_cases.CODES["short"], 2
    P, d = 32 + 8 * code.n * I, 32
    pad = frame_sync.ccsds_randomizer(code.n * I)
    n_frames = 4
    rng = np.random.default_rng(8)
    rows, sents = [], []
    for lead in (100, 777):
        sent = rs_encode_numpy(code, rng.integers(0, 256, size=(n_frames, code.k * I), dtype=np.uint8), I)
        got = sent.copy()
        for m in range(n_frames):
            for c in range(I):
                rs_cases.ref.corrupt(rng, got[m], I, c, [0, code.t, code.t + 3, 5][(m + c) % 4])
        mk = np.array([(CCSDS_ASM[0] >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)
        frames = np.concatenate([np.broadcast_to(mk, (n_frames, 32)), np.unpackbits(got ^ pad, axis=1)], axis=1)
        rows.append(np.packbits(np.concatenate([rng.integers(0, 2, size=lead, dtype=np.uint8), frames.reshape(-1),
                                                rng.integers(0, 2, size=900 - lead, dtype=np.uint8)])))
        sents.append((got, lead))
    n_bits = 900 + n_frames * P
    d_bytes = torch.from_numpy(rows[0]).cuda()
    d_pad = torch.from_numpy(pad).cuda()
    lock = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    cap = dec.frames_capacity(n_bits, P)
    out = (torch.empty((1, cap, code.n * I), dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
           torch.empty((1, cap), dtype=torch.int32, device="cuda"), torch.empty((1, (P + 6) // 8), dtype=torch.uint8, device="cuda"),
           torch.empty(1, dtype=torch.int32, device="cuda"))
    status = torch.empty((1, cap, I), dtype=torch.int32, device="cuda")

    def chain():
        dec.frames_extract(d_bytes, n_bits, P, 0, lock, marker=CCSDS_ASM[0], marker_bits=32, drop_bits=d, pad=d_pad, out=out)
        dec.rs_decode(code, out[0], out[1], I, status=status)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for row, (got, lead) in zip(rows, sents):
        d_bytes.copy_(torch.from_numpy(row).cuda())
        lock.copy_(torch.tensor([[lead, 0, 0, 0]], dtype=torch.int32))
        out[0].fill_(POISON)
        status.fill_(int(POISON32))
        graph.replay()
        torch.cuda.synchronize()
        assert int(out[1].item()) == n_frames
        want, want_status = rs_cases.ref.decode(code, got, I)
        assert (want_status == -1).any() and (want_status > 0).any()
        assert np.array_equal(status[0, :n_frames].cpu().numpy(), want_status) and np.array_equal(out[0][0, :n_frames].cpu().numpy(), want)
        assert (out[0][0, n_frames:] == POISON).all().item() and (status[0, n_frames:] == int(POISON32)).all().item()


CHAIN_SEED = 39       # chosen by the channel alone: behind the Viterbi decoder this noise leaves bit errors for the outer code


def chain_case(seed, code, I, n_frames, ebn0_db, streams=1):
    """payload -> RS -> randomiser -> ASM -> K = 7 R = 1/2 -> the project's channel (BPSK + noise, scaled and clamped to [low, high];
    None: no noise), per stream.  returns (bits [streams][n], payload [streams][n_frames][k I], clean symbols, received symbols
    [streams][steps][R], pad, P)"""
    import torch
    conv, pc, dec = decoder()
    P = 32 + 8 * code.n * I
    rng = np.random.default_rng(seed)
    payload = rng.integers(0, 256, size=(streams, n_frames, code.k * I), dtype=np.uint8)
    sent = rs_encode_numpy(code, payload, I)
    pad = frame_sync.ccsds_randomizer(code.n * I)
    mk = np.array([(CCSDS_ASM[0] >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)
    bits = np.concatenate([np.broadcast_to(mk, (streams, n_frames, 32)), np.unpackbits(sent ^ pad, axis=2)], axis=2).reshape(streams, -1)
    sym = dec.encode(torch.from_numpy(np.packbits(bits, axis=1)).cuda(), bits.shape[1], tail=True).cpu().numpy()
    mid = (pc.soft_decision_high + pc.soft_decision_low) / 2
    noisy = synth.quantise_numpy((sym > mid).astype(np.uint8), pc.soft_decision_high, pc.soft_decision_low, ebn0_db, conv.R, rng, pc.soft_dtype)
    return bits, payload, sym, noisy, pad, P


def emitted_per_call(rx):
    K = decoder()[0].K
    sizes = [steps - (K - 1 if end else rx.tail) - (0 if begin else rx.head) for steps, begin, end in rx.calls]
    assert sum(sizes) == rx.n_bits
    return sizes


def test_the_whole_chain_through_the_stream_decoder_at_3_db():
    """payload -> RS (dual basis) -> randomiser -> ASM -> K = 7 R = 1/2 -> noise -> StreamDecoder with marker, frames and rs"""
    import torch
    conv, pc, dec = decoder()
    code, I, n_frames, d = CCSDS_RS_255_223_DUAL, 1, 8, 32
    bits, payload, sym, noisy, pad, P = chain_case(CHAIN_SEED, code, I, n_frames, 3.0)
    bits, payload, sym, noisy = bits[0], payload[0], sym[0], noisy[0]
    mid = (pc.soft_decision_high + pc.soft_decision_low) / 2
    d_sym = torch.from_numpy(noisy).cuda()
    assert ((noisy > mid) != (sym > mid)).mean() > 0.05                     # the channel does flip symbols
    rx = StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=d, frame_pad=pad, rs=code)
    cut = 3 * P * 2 + 111 * 2
    cut -= cut % conv.R
    data = rx.push(d_sym.reshape(-1)[:cut])
    first = rx.take_frames()
    data += rx.finish(d_sym.reshape(-1)[cut:])
    second = rx.take_frames()
    decoded = np.unpackbits(np.frombuffer(data, dtype=np.uint8))[:rx.n_bits]
    assert rx.n_bits == bits.size
    print("bit errors behind the Viterbi decoder:", int((decoded != bits).sum()))
    # the chain on the CPU, by the numpy rules, delivers every frame: the test cannot hide a loss
    cpu_frames, cpu_errors, _ = fr.receiver_numpy(decoded, emitted_per_call(rx), *CCSDS_ASM, P, d, pad)
    cpu_out, cpu_status = rs_decode_numpy(code, cpu_frames, I)
    assert len(cpu_frames) == n_frames and (cpu_status >= 0).all() and np.array_equal(cpu_out[:, :code.k], payload)
    print("byte errors corrected per frame:", cpu_status.reshape(-1).tolist())
    assert (cpu_status > 0).any()                                           # the seed leaves the outer code something to correct
    frames = np.concatenate([first[0], second[0]])
    errors, status = np.concatenate([first[1], second[1]]), np.concatenate([first[2], second[2]])
    assert len(first[0]) >= 2 and len(second[0]) >= 2 and status.dtype == np.int32 and status.shape == (n_frames, I)
    assert np.array_equal(status, cpu_status) and np.array_equal(frames, cpu_out) and np.array_equal(errors, cpu_errors)
    good = status[:, 0] >= 0
    assert good.all() and np.array_equal(frames[good][:, :code.k], payload[good])
    # without rs= nothing changes: the 2-tuple
    plain = StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=d, frame_pad=pad)
    plain.push(d_sym.reshape(-1)[:cut])
    plain.finish(d_sym.reshape(-1)[cut:])
    taken = plain.take_frames()
    assert len(taken) == 2 and np.array_equal(taken[0], cpu_frames)
    with pytest.raises(ValueError):
        StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P + 8, frames=True, frame_drop_bits=d, rs=code)
    with pytest.raises(ValueError):
        StreamDecoder(dec, 1024, marker=CCSDS_ASM, period=P, rs=code)


def test_multi_stream_decoder_decodes_the_codewords_of_every_stream():
    """two streams of CCSDS frames at interleave depth 5 with byte errors put in behind the RS encoder: 0 .. t in most codewords, more
    than t in one; ragged pushes; the status per stream and codeword, and the empty triple"""
    import torch
    conv, pc, dec = decoder()
    code, I, n_frames, d = CCSDS_RS_255_223_DUAL, 5, 3, 32
    rng = np.random.default_rng(12)
    P = 32 + 8 * code.n * I
    payload = rng.integers(0, 256, size=(2, n_frames, code.k * I), dtype=np.uint8)
    sent = rs_encode_numpy(code, payload, I)
    got = sent.copy()
    for i in range(2):
        for m in range(n_frames):
            for c in range(I):
                rs_cases.ref.corrupt(rng, got[i, m], I, c, code.t + 4 if (i, m, c) == (1, 1, 3) else (i + m + 3 * c) % (code.t + 1))
    pad = frame_sync.ccsds_randomizer(code.n * I)
    mk = np.array([(CCSDS_ASM[0] >> (31 - j)) & 1 for j in range(32)], dtype=np.uint8)
    bits = np.concatenate([np.broadcast_to(mk, (2, n_frames, 32)), np.unpackbits(got ^ pad, axis=2)], axis=2).reshape(2, -1)
    d_sym = dec.encode(torch.from_numpy(np.packbits(bits, axis=1)).cuda(), bits.shape[1], tail=True)
    rx = MultiStreamDecoder(dec, 2, 1024, marker=CCSDS_ASM, period=P, frames=True, frame_drop_bits=d, frame_pad=pad, rs=code, rs_interleave=I)
    empty = rx.take_frames()
    assert [tuple(x.shape) for x in empty[1]] == [(0, code.n * I), (0,), (0, I)] and empty[1][2].dtype == np.int32
    taken = [[], []]
    cuts = [0, P * 2 + 500, P * 2 + 7000, d_sym.shape[1]]
    for a, b in zip(cuts[:-1], cuts[1:]):
        rx.push(d_sym[:, a:b]) if b < d_sym.shape[1] else rx.finish(d_sym[:, a:b])
        for i, t3 in enumerate(rx.take_frames()):
            assert len(t3) == 3 and len(t3[0]) == len(t3[1]) == len(t3[2])
            taken[i].append(t3)
    assert sum(len(t3[0]) > 0 for t3 in taken[0]) >= 2                       # the frames came out over more than one take
    for i in range(2):
        frames, errors, status = (np.concatenate([t3[k] for t3 in taken[i]]) for k in range(3))
        want, want_status = rs_cases.ref.decode(code, got[i], I)
        assert status.shape == (n_frames, I) and np.array_equal(status, want_status) and np.array_equal(frames, want)
        assert not errors.any()
        good = (status >= 0).all(axis=1)
        assert np.array_equal(frames[good], sent[i][good]) and (status[good] > 0).any()
    assert want_status[1, 3] == -1 and (want_status >= 0).sum() == n_frames * I - 1
