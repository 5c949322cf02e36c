"""The 802.11a/g data path on the GPU at the shapes tests/test_gpu_wifi.py never reaches, bit for bit against the numpy rules of
viterbidecodercpp_amd/wifi.py (pinned to tests/wifi_reference.py by tests/test_wifi_cpu.py), every output over a fill pattern with a
64-element guard behind it, every input compared with what was uploaded:
  A  the de-interleaver at (frames, S) in {1, 3, 5, 31, 257} x {1, 2, 3, 37, 433} on SOFT8, HARD8 and SOFT16 handles, at one rate and
     mixed through d_rate with rates of 8 and above: on the one-byte handles the odd x odd shapes leave two elements behind the last whole
     dword, which threads of block 0 store one by one, and (1, 1) has no whole dword at all;
  B  the DATA kernel at one max_length per (lanes of a frame, bytes of a chunk) crc_geometry can give, one frame per LENGTH, at every
     alignment of d_bytes and of d_psdu with odd strides: every LENGTH 4 .. 7 (the FCS register's init carried past a message shorter
     than four octets), every count of bytes in front of octet 0 in a lane's first word, both store paths;
  C  all 128 values of the first seven decoded bits, 0 among them, with lengths that put a window of the 127-bit sequence at every
     position, and SERVICE fields that are not zero;
  D  all 2^18 SIGNAL fields;
  E  the whole WifiDecoder chain at SOFT16 and SOFT8 on PPDUs of which a third fail -- SIGNAL fields no sender may send, SIGNAL and DATA
     fields lost in noise --, directly and replayed from a captured graph: the reference is the bit-exact oracle decoder, so a frame that
     fails is compared like one that passes."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from viterbidecodercpp_amd import (WIFI_RATES, WifiDecoder, _lib, wifi_deinterleave_numpy, wifi_descramble_numpy, wifi_scrambler_numpy,
                                   wifi_signal_parse_numpy)
from tests import wifi_cases as cases
from tests.test_gpu_wifi import (CHAIN_MAX_SYM, FILL8, GUARD, check_descramble, decoder, ptr, run_deinterleave, side_stream, soft_bits, u32)

pytestmark = pytest.mark.gpu


# ---- A: de-interleaver tails and tiny shapes -------------------------------------------------------------------------------------------------

DEINT_FRAMES, DEINT_S, DEINT_MAX_SYM = (1, 3, 5, 31, 257), (1, 2, 3, 37, 433), 3
HOSTILE_RATES = (0, 8, 1, 2, 2 ** 32 - 1, 3, 4, 9, 5, 6, 7)          # a frame erased whole between two that are not


def one_rate_of(S):
    """the rate of the one-rate call at S: all eight over the five S, 54 Mbit/s at S = 433, where only 3 * 216 steps reach past S.  The
    last step is then sent in both outputs (q = 2 S - 2 and 2 S - 1 are 0 and 1 mod 6 at S = 37 and 433, the rate 3/4 ones)"""
    return {1: 0, 2: 6, 3: 4, 37: 3, 433: 7}[S]


@functools.lru_cache(maxsize=None)
def deint_case(dtype, frames, S, mixed):
    """(soft, keyword arguments of the rule and of run_deinterleave, what the rule gives) -- computed once for the handles that share a dtype"""
    rng = np.random.default_rng(1000 * frames + S)
    soft = soft_bits(rng, dtype, (frames, DEINT_MAX_SYM * 288))
    if mixed:
        rates = [HOSTILE_RATES[(f + S) % len(HOSTILE_RATES)] for f in range(frames)]
        n_sym = [(3, 1, 2, 2 ** 32 - 1, 4, 0, 3)[(f + frames) % 7] for f in range(frames)]
        full = [min(n_sym[f], DEINT_MAX_SYM) * WIFI_RATES[m].n_dbps if m < 8 else 0 for f, m in enumerate(rates)]
        # inside a puncturing period (full - 1, - 2, S - 1, an odd count), above everything, none at all
        n_steps = [max((full[f], full[f] - 1, S - 1, full[f] - 2, 2 ** 32 - 1, 7, 0, S)[f % 8], 0) for f in range(frames)]
        kw = dict(rates=rates, n_sym=n_sym, n_steps=n_steps)
    else:
        # the last frame whole, so that the elements behind the last dword are soft bits and not erasures
        n_steps = [(S, 2 ** 32 - 1, max(S - 1, 0), max(S - 2, 0), 7, S + 1)[(frames - 1 - f) % 6] for f in range(frames)]
        kw = dict(rate=one_rate_of(S), n_steps=n_steps)
    rule = {("rate" if k == "rates" else k): v for k, v in kw.items()}           # the rule takes the per-frame rates as `rate`
    want = wifi_deinterleave_numpy(soft, DEINT_MAX_SYM, S, **rule)
    soft.setflags(write=False), want.setflags(write=False)
    return soft, kw, want


@pytest.mark.parametrize("mixed", [False, True], ids=["one_rate", "d_rate"])
@pytest.mark.parametrize("decode_type,dtype", [("SOFT8", np.int8), ("HARD8", np.int8), ("SOFT16", np.int16)])
def test_the_deinterleaver_behind_the_last_dword(decode_type, dtype, mixed):
    """run_deinterleave checks the 64 guard elements from the one directly behind the last output on: a tail that stores one element too
    many is seen there"""
    dec = decoder(decode_type)
    tails = 0
    for frames in DEINT_FRAMES:
        for S in DEINT_S:
            soft, kw, want = deint_case(dtype, frames, S, mixed)
            total = frames * 2 * S
            if dtype == np.int8 and frames % 2 and S % 2:
                assert total % 4 == 2                              # the two elements that block 0 stores one by one ...
                assert mixed or want.reshape(-1)[-2:].all()        # ... and they are soft bits in the one-rate call
                assert total // 4 or (frames, S) == (1, 1)         # no whole dword at all only at (1, 1)
                tails += 1
            else:
                assert total * np.dtype(dtype).itemsize % 4 == 0
            for cs in ((1, 3) if mixed else (1,)):
                got = run_deinterleave(dec, np.asarray(soft), DEINT_MAX_SYM, S, count_stride=cs, **kw)
                assert np.array_equal(got, want), (frames, S, cs)
            assert want.any() or frames == 1
    assert tails == (20 if dtype == np.int8 else 0)
    if mixed:                                                      # an erased frame and a valid one in ONE dword: S = 1, two frames a dword
        soft, kw, want = deint_case(dtype, 31, 1, True)
        assert any(not want[f].any() and want[f + 1].all() and f % 2 == 0 for f in range(30)) or dtype == np.int16
        assert [m for m in kw["rates"] if m > 7]


# ---- B: the DATA kernel at every geometry -------------------------------------------------------------------------------------------------------

def geometry(max_len):
    """crc_geometry (csrc/kernels_crc.hpp) for the FCS message of the longest PSDU a call allows: len - 4 octets right-aligned in 2^logG
    chunks of C bytes; the lanes double while a chunk would be longer than 16 bytes, up to 64, and C is the chunk rounded up to dwords"""
    octets = max(max_len - 4, 0)
    logG = 0
    while (1 << logG) < 64 and -(-octets // (1 << logG)) > 16:
        logG += 1
    per = -(-octets // (1 << logG))
    return logG, (per + 3) // 4 * 4 if per else 4


def geometry_lengths():
    """the LARGEST max_length of every distinct (logG, C): {(logG, C): max_length}"""
    out = {}
    for n in range(4096):
        out[geometry(n)] = n
    return out


GEOMETRIES = geometry_lengths()
DATA_SEEDS = (1, 127, 0x55, 93, 64, 3, 0x2A, 8)


def test_the_geometries_listed():
    assert {g[0] for g in GEOMETRIES} == set(range(7))
    assert {g[1] for g in GEOMETRIES} == set(range(4, 68, 4))
    assert GEOMETRIES[(0, 4)] == 8 and GEOMETRIES[(6, 64)] == 4095 and len(GEOMETRIES) == 28
    assert all(geometry(n) == g for g, n in GEOMETRIES.items())


@functools.lru_cache(maxsize=None)
def sequence(seed):
    """wifi_scrambler_numpy over the longest frame, once per seed"""
    s = wifi_scrambler_numpy(seed, 8 * (4095 + 3))
    s.setflags(write=False)
    return s


def lengths_of(max_length, C):
    if max_length < 300:
        return list(range(max_length + 3))
    near = [k * C + d for k in range(max_length // C + 2) for d in range(-3, 8)]       # LENGTH and LENGTH - 4 within 3 of a multiple of C
    return sorted({n for n in list(range(41)) + near + list(range(max_length - 39, max_length + 3)) if 0 <= n <= max_length + 2})


@functools.lru_cache(maxsize=4)
def data_case(max_length):
    """one frame per LENGTH: decoded bytes [frames][max_length + 3] (what S = 22 + 8 max_length + 7 holds), the LENGTHs, and what the call
    must give, from how the frames were made: the PSDU image, the status.  A PSDU of four octets or more carries its FCS; every third has
    one bit flipped behind that, in its body (in the FCS where there is no body)"""
    C_ = geometry(max_length)[1]
    lengths = lengths_of(max_length, C_)
    rng = np.random.default_rng(max_length)
    n_bits = 8 * (max_length + 3)
    data = np.zeros((len(lengths), max_length + 3), dtype=np.uint8)
    image = np.full((len(lengths), max(max_length, 1)), FILL8, dtype=np.uint8)
    status = np.zeros((len(lengths), 4), dtype=np.uint32)
    for f, length in enumerate(lengths):
        n = min(length, max_length)
        body = rng.integers(0, 256, size=max(n - 4, 0) if n >= 4 else n, dtype=np.uint8)
        psdu = (cases.with_fcs(body.tobytes()) if n >= 4 else body).copy()
        if n >= 4 and f % 3 == 2:
            at = int(rng.integers(0, 8 * (n - 4))) if n > 4 else int(rng.integers(0, 32))
            psdu[at // 8] ^= 1 << (at % 8)
        seed = DATA_SEEDS[f % len(DATA_SEEDS)]
        service = (int(rng.integers(0, 2 ** 16)) & 0xFF80) if f % 4 == 1 else 0        # bits 0 .. 6 initialise the scrambler: zero
        bits = rng.integers(0, 2, size=n_bits, dtype=np.uint8)                        # pad and tail: anything
        bits[:16] = (service >> np.arange(16)) & 1
        bits[16:16 + 8 * n] = np.unpackbits(psdu, bitorder="little")
        data[f] = np.packbits(bits ^ sequence(seed)[:n_bits])
        image[f, :n] = psdu
        syndrome = 0xFFFFFFFF
        if n >= 4:
            syndrome = zlib.crc32(psdu[:n - 4].tobytes()) ^ int.from_bytes(psdu[n - 4:].tobytes(), "little")
            assert (syndrome != 0) == (f % 3 == 2)                 # the expected class: it checks, or one flipped bit shows
        status[f] = (n, seed, service, syndrome)
    for x in (data, image, status):
        x.setflags(write=False)
    return data, lengths, image, status


def run_data_at(dec, data, S, lengths, max_length, in_off, in_stride, ps_off, ps_stride):
    """vit_hip_wifi_data_batch with d_bytes in_off bytes and d_psdu ps_off bytes into their allocations -> (psdu image [frames][ps_stride],
    status uint32 [frames][4]); the bytes in front of d_psdu, the guards behind both outputs and the input checked"""
    import torch
    frames, nb = data.shape
    host = np.random.default_rng(in_off).integers(0, 256, size=in_off + frames * in_stride, dtype=np.uint8)
    rows = host[in_off:].reshape(frames, in_stride)
    rows[:, :nb] = data
    d_in = torch.from_numpy(host).cuda()
    d_psdu = torch.full((ps_off + frames * ps_stride + GUARD,), FILL8, dtype=torch.uint8, device="cuda")
    d_status = torch.full((frames * 4 + GUARD,), -1, dtype=torch.int32, device="cuda")
    d_len = u32(lengths)
    rc = _lib.load().vit_hip_wifi_data_batch(dec._handle._h, ptr(d_in, in_off), in_stride, frames, S, ptr(d_len), 1, max_length,
                                             ptr(d_psdu, ps_off), ps_stride, ptr(d_status), None)
    assert rc == _lib.OK, _lib.load().vit_hip_last_error()
    torch.cuda.synchronize()
    psdu, status = d_psdu.cpu().numpy(), d_status.cpu().numpy()
    assert (psdu[:ps_off] == FILL8).all() and (psdu[ps_off + frames * ps_stride:] == FILL8).all() and (status[frames * 4:] == -1).all()
    assert np.array_equal(d_in.cpu().numpy(), host)
    return psdu[ps_off:ps_off + frames * ps_stride].reshape(frames, ps_stride), status[:frames * 4].view(np.uint32).reshape(frames, 4)


@pytest.mark.parametrize("logG,C_", sorted(GEOMETRIES))
def test_the_data_kernel_at_every_geometry_and_length(logG, C_):
    dec = decoder("SOFT16")
    max_length = GEOMETRIES[(logG, C_)]
    data, lengths, image, status = data_case(max_length)
    nb = data.shape[1]
    assert status[[n < 4 for n in lengths], 3].tolist() == [0xFFFFFFFF] * min(4, len(lengths))
    assert set(range(min(8, max_length + 1))) <= set(lengths)       # LENGTH 4 .. 7: a message below four octets, where there is room
    # the rule itself, against how the frames were made: all frames of the short geometries, a spread of the long ones
    some = np.arange(len(lengths)) if max_length < 300 else np.unique(np.linspace(0, len(lengths) - 1, 24).astype(int))
    S_rule = 22 + 8 * max_length + 7
    octets, st = wifi_descramble_numpy(data[some], S_rule, np.asarray(lengths)[some], max_length)
    assert np.array_equal(st, status[some])
    assert all(o.tobytes() == image[f, :o.size].tobytes() and o.size == status[f, 0] for f, o in zip(some, octets))
    in_stride, ps_stride = (nb + 2) | 1, max(max_length, 1) | 1     # odd: a frame's alignment differs from its neighbour's
    want = np.full((len(lengths), ps_stride), FILL8, dtype=np.uint8)
    want[:, :image.shape[1]] = image
    chunk = 150 if max_length >= 300 else len(lengths)
    call = 0
    for in_off in range(4):
        for ps_off in range(4):
            S = 22 + 8 * max_length + (0, 1, 7)[call % 3]
            assert (S - 6) % 8 in (0, 1, 7) and (S - 22) // 8 == max_length
            allowed = (max_length, 4095, max_length + 1)[call % 3]          # the call's max_length: the geometry comes from what S holds too
            assert geometry(min(allowed, (S - 22) // 8)) == (logG, C_)
            call += 1
            for lo in range(0, len(lengths), chunk):
                got_psdu, got_status = run_data_at(dec, data[lo:lo + chunk], S, lengths[lo:lo + chunk], allowed, in_off, in_stride, ps_off, ps_stride)
                assert np.array_equal(got_status, status[lo:lo + chunk]), (in_off, ps_off, S)
                assert np.array_equal(got_psdu, want[lo:lo + chunk]), (in_off, ps_off, S)


# ---- C: every seed, every position of the sequence ----------------------------------------------------------------------------------------

def window_starts(max_len, msg):
    """where in the 127-bit sequence the first word of every lane's chunk starts, as wifi_data_chunk places the chunks: the message of msg
    octets right-aligned in G chunks of C bytes, a lane's first word the one that holds its first message bit"""
    logG, C_ = geometry(max_len)
    G, out = 1 << logG, []
    for j in range(G):
        p0 = 8 * msg - (G - j) * 8 * C_
        k0 = (-p0) >> 5 if p0 < 0 else 0
        if msg and k0 < C_ // 4:
            out.append((16 + p0 + 32 * k0) % 127)
    return out


def test_every_seed_and_every_position_of_the_sequence():
    dec = decoder("SOFT16")
    rng = np.random.default_rng(6)
    max_length = 260
    S = 22 + 8 * max_length + 1
    assert geometry(max_length) == (4, 16)
    lengths = [104 + f for f in range(128)]
    starts = {p for n in lengths for p in window_starts(max_length, n - 4)}
    assert starts == set(range(127))
    services = [(0x0280 * f) & 0xFF80 if f % 3 == 1 else 0 for f in range(128)]
    rows = []
    for f, n in enumerate(lengths):
        bits = rng.integers(0, 2, size=S - 6, dtype=np.uint8)
        bits[:16] = (services[f] >> np.arange(16)) & 1
        psdu = cases.with_fcs(rng.integers(0, 256, size=n - 4, dtype=np.uint8).tobytes())
        bits[16:16 + 8 * n] = np.unpackbits(psdu, bitorder="little")
        rows.append(np.packbits(bits ^ wifi_scrambler_numpy(f, S - 6)))            # seed f; 0: the scrambled bits are the bits
    data = np.stack(rows)
    assert not wifi_scrambler_numpy(0, 127).any() and data[0, 0] >> 1 == 0
    status = check_descramble(dec, data, S, lengths, max_length, psdu_stride=261)
    assert status[:, 1].tolist() == list(range(128)) and status[:, 2].tolist() == services and any(services)
    assert status[:, 0].tolist() == lengths and not status[:, 3].any()


# ---- D: every SIGNAL field -----------------------------------------------------------------------------------------------------------------

def test_every_signal_field():
    import torch
    dec = decoder("SOFT16")
    rng = np.random.default_rng(7)
    v = np.arange(2 ** 18, dtype=np.uint32) << 6 | rng.integers(0, 64, size=2 ** 18).astype(np.uint32)       # the six tail bits: anything
    fields = np.stack([v >> 16, v >> 8, v], axis=1).astype(np.uint8)
    want = wifi_signal_parse_numpy(fields)
    assert int(want[:, 4].sum()) == 8 * 4095
    for stride in (3, 5):
        host = rng.integers(0, 256, size=(2 ** 18, stride), dtype=np.uint8)
        host[:, :3] = fields
        d = torch.from_numpy(host).cuda()
        out = torch.full((2 ** 18 * 5 + GUARD,), -1, dtype=torch.int32, device="cuda")
        rc = _lib.load().vit_hip_wifi_signal_batch(dec._handle._h, ptr(d), stride, 2 ** 18, ptr(out), None)
        assert rc == _lib.OK, _lib.load().vit_hip_last_error()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:2 ** 18 * 5].view(np.uint32).reshape(-1, 5), want) and (got[2 ** 18 * 5:] == -1).all()
        assert np.array_equal(d.cpu().numpy(), host)


# ---- E: the chain where frames fail, and at SOFT8 -----------------------------------------------------------------------------------------------

# 64 PPDUs; every third one in noise of 0.7 .. 1.4 of the amplitude, where SIGNAL or the FCS fails; eight SIGNAL fields no sender may send
FAIL_SPECS = [(f % 8, 4 + (41 * f) % (cases.largest_length(f % 8, CHAIN_MAX_SYM) - 3), 1 + (31 * f) % 127) for f in range(64)]
FAIL_SIGMA = [0.7 + 0.1 * (f // 3 % 8) if f % 3 == 1 else 0.2 for f in range(64)]
FAIL_SEEDS = (11, 12)                                               # of make_ppdus: chosen on the CPU so that fail_case's conditions hold


def bad_signal_fields():
    """{frame: 18 bits}: a bad parity, the reserved bit set (parity right), LENGTH 0, a rate pattern that is none of the eight -- twice each"""
    out = {}
    for f in (0, 9, 18, 27, 36, 45, 54, 63):
        rate, length, _ = FAIL_SPECS[f]
        bits = cases.signal_bits(rate, length)
        kind = f // 9 % 4
        if kind == 0:
            bits[17] ^= 1
        elif kind == 1:
            bits[4] = 1
            bits[17] ^= 1
        elif kind == 2:
            bits = cases.signal_bits(rate, 0)
        else:
            bits[:4] = ((0, 0, 0, 0), (1, 1, 1, 0))[f // 36]
            bits[17] = bits[:17].sum() % 2
        out[f] = bits
    return out


@functools.lru_cache(maxsize=None)
def fail_case(decode_type, seed):
    signal_soft, data_soft, psdus = cases.make_ppdus(FAIL_SPECS, CHAIN_MAX_SYM, seed=seed, sigma=FAIL_SIGMA, decode_type=decode_type,
                                                     signal_bits18=bad_signal_fields())
    image, status, signal = cases.cpu_chain(signal_soft, data_soft, CHAIN_MAX_SYM, decode_type)
    # conditions on the input, checked on the CPU side
    bad = sorted(bad_signal_fields())
    assert not signal[bad, 4].any() and not signal[bad, 3].any()
    invalid = signal[:, 4] == 0
    failed = (signal[:, 4] == 1) & (status[:, 3] != 0)
    clean = (signal[:, 4] == 1) & (status[:, 3] == 0) & (status[:, 2] == 0)
    print(decode_type, seed, "invalid", int(invalid.sum()), "FCS failed", int(failed.sum()), "clean", int(clean.sum()))
    assert invalid.sum() >= 8 and failed.sum() >= 8 and clean.sum() >= 16
    assert (signal[:, 4] == 1)[np.asarray(FAIL_SIGMA) > 0.5].any() and invalid.sum() > 8        # noise alone breaks SIGNAL fields too
    for f in np.flatnonzero(clean):
        assert image[f, :psdus[f].size].tobytes() == psdus[f].tobytes() and status[f, 0] == psdus[f].size
    for x in (signal_soft, data_soft, image, status, signal):
        x.setflags(write=False)
    return signal_soft, data_soft, image, status, signal


def chain_outputs(shape):
    import torch
    return (torch.full(shape, cases.FILL, dtype=torch.uint8, device="cuda"), torch.full((64, 4), -1, dtype=torch.int32, device="cuda"),
            torch.full((64, 5), -1, dtype=torch.int32, device="cuda"))


def assert_chain(out, case):
    signal_soft, data_soft, image, status, signal = case
    assert np.array_equal(out[2].cpu().numpy().view(np.uint32), signal)
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), status)
    assert np.array_equal(out[0].cpu().numpy(), image)             # the fill behind every frame's length_used included


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_the_chain_where_frames_fail(decode_type):
    import torch
    case = fail_case(decode_type, FAIL_SEEDS[0])
    wifi = WifiDecoder(decoder(decode_type), decoder(decode_type), CHAIN_MAX_SYM)
    assert wifi.max_length == case[2].shape[1]
    d_signal, d_data = torch.from_numpy(case[0].copy()).cuda(), torch.from_numpy(case[1].copy()).cuda()
    out = wifi.decode(d_signal, d_data, out=chain_outputs(case[2].shape))
    torch.cuda.synchronize()
    assert_chain(out, case)
    assert np.array_equal(d_signal.cpu().numpy(), case[0]) and np.array_equal(d_data.cpu().numpy(), case[1])


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_the_failing_chain_replayed_from_a_graph(decode_type):
    """captured as tests/test_gpu_wifi.py captures, on that test's side stream; replayed on input it was not captured with"""
    import torch
    wifi = WifiDecoder(decoder(decode_type), decoder(decode_type), CHAIN_MAX_SYM)
    first = fail_case(decode_type, FAIL_SEEDS[0])
    d_signal, d_data = torch.from_numpy(first[0].copy()).cuda(), torch.from_numpy(first[1].copy()).cuda()
    out = chain_outputs(first[2].shape)
    side = side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wifi.decode(d_signal, d_data, out=out)                     # warm-up outside the capture: every buffer is allocated here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wifi.decode(d_signal, d_data, out=out)
    for seed in FAIL_SEEDS[::-1]:
        case = fail_case(decode_type, seed)
        d_signal.copy_(torch.from_numpy(case[0].copy()).cuda()), d_data.copy_(torch.from_numpy(case[1].copy()).cuda())
        out[0].fill_(cases.FILL), out[1].fill_(-1), out[2].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert_chain(out, case)
