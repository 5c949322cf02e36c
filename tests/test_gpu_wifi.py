"""The 802.11a/g data path on the GPU: vit_hip_wifi_deinterleave_batch, vit_hip_wifi_signal_batch and vit_hip_wifi_data_batch against the
numpy rules of viterbidecodercpp_amd/wifi.py, byte for byte over a fill pattern, written or not -- all eight rates in ONE call through
d_rate with 1 .. 3 symbols mixed, step counts cut inside a puncturing period and inside an OFDM symbol, invalid rates, a non-default
stride, the per-frame arguments read out of SIGNAL structs, one frame (also through the Python layer with the output placed right behind
the input), one frame of LENGTH 4095 at 6 Mbit/s (1366 symbols), SOFT16 and
SOFT8 handles; the descrambler at lengths 0, 3, 4, 5, 63, 64, 65, 4095, an all-zero first seven bits, a length above what the frame holds
and a corrupted FCS; the rejections; the whole WifiDecoder chain on 64 noisy PPDUs of mixed rate and length against the CPU composition,
and the same chain captured into a graph and replayed."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, WIFI_POLYNOMIALS, WIFI_RATES, BatchDecoder, WifiDecoder, _lib, wifi_deinterleave_numpy,
                                   wifi_descramble_numpy, wifi_scrambler_numpy, wifi_signal_parse_numpy)
from tests import wifi_cases as cases
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

GUARD = 64
FILL16, FILL8 = 0x5A5A, 0x5A


@functools.lru_cache(maxsize=None)
def decoder(decode_type="SOFT16", code_index=2):
    code = COMMON_CODES[code_index]
    pc, table, config = make_table_config(code, decode_type)
    return BatchDecoder(table, config)


def test_the_stock_code_serves_the_polynomials():
    assert tuple(COMMON_CODES[2].G) == WIFI_POLYNOMIALS and (COMMON_CODES[2].K, COMMON_CODES[2].R) == (7, 2)


def ptr(x, byte_offset=0):
    return None if x is None else C.c_void_p(x.data_ptr() + byte_offset)


def u32(values, stride=1):
    """uint32 values on the device, entry f at element f * stride, noise between them"""
    import torch
    a = np.random.default_rng(len(values)).integers(0, 2 ** 32, size=(len(values) - 1) * stride + 1, dtype=np.uint64).astype(np.uint32)
    a[::stride] = np.asarray(values, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


def run_deinterleave(dec, soft, max_sym, S, rate=0, rates=None, n_sym=None, n_steps=None, count_stride=1, stride=0):
    """the call through the C ABI -> [frames][S][2] as numpy, after the guard behind the output and the input have been checked; compared
    by the caller with the numpy rule"""
    import torch
    frames = soft.shape[0]
    fill = FILL16 if soft.dtype == np.int16 else FILL8
    d_in = torch.from_numpy(soft.copy()).cuda()
    buf = torch.full((frames * S * 2 + GUARD,), fill, dtype=d_in.dtype, device="cuda")
    arrays = [None if x is None else u32(x, count_stride) for x in (rates, n_sym, n_steps)]
    rc = _lib.load().vit_hip_wifi_deinterleave_batch(dec._handle._h, ptr(d_in), stride, frames, max_sym, rate, ptr(arrays[0]), ptr(arrays[1]),
                                                     ptr(arrays[2]), count_stride, S, ptr(buf), None)
    assert rc == _lib.OK, _lib.load().vit_hip_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[frames * S * 2:] == fill).all()
    assert np.array_equal(d_in.cpu().numpy(), soft)
    return got[:frames * S * 2].reshape(frames, S, 2)


def soft_bits(rng, dtype, shape):
    lo, hi = (-32768, 32767) if dtype == np.int16 else (-128, 127)
    x = rng.integers(lo, hi + 1, size=shape)
    return np.where(x == 0, 1, x).astype(dtype)                    # no zero among the inputs: a zero in the output is an erasure


@pytest.mark.parametrize("decode_type,dtype", [("SOFT16", np.int16), ("SOFT8", np.int8)])
def test_all_rates_in_one_call(decode_type, dtype):
    dec = decoder(decode_type)
    rng = np.random.default_rng(1)
    max_sym = 3
    rates = [0, 1, 2, 3, 4, 5, 6, 7] * 3 + [8, 2 ** 32 - 1, 9, 7, 6, 1]
    F = len(rates)
    n_sym = [1 + f % 3 for f in range(F)]
    n_sym[3], n_sym[4] = 0, 2 ** 32 - 1
    full = [min(n_sym[f], max_sym) * WIFI_RATES[m].n_dbps if m < 8 else 0 for f, m in enumerate(rates)]
    # inside a puncturing period (full - 1, - 2, an odd count), inside an OFDM symbol (N_DBPS + 5), above everything, none at all
    n_steps = [(full[f], full[f] - 1, full[f] - 2, WIFI_RATES[min(m, 7)].n_dbps + 5, 2 ** 32 - 1, 7, 0)[f % 7] for f, m in enumerate(rates)]
    soft = soft_bits(rng, dtype, (F, max_sym * 288))
    for S in (max_sym * 216, 2 * 216 + 1, 37):                     # S odd: at soft8 a dword holds symbols of two frames
        want = wifi_deinterleave_numpy(soft, max_sym, S, rate=rates, n_sym=n_sym, n_steps=n_steps)
        for cs in (1, 5):
            got = run_deinterleave(dec, soft, max_sym, S, rates=rates, n_sym=n_sym, n_steps=n_steps, count_stride=cs)
            assert np.array_equal(got, want), (S, cs)
        assert want.any() and not want[24:27].any()
    want = wifi_deinterleave_numpy(soft, max_sym, max_sym * 216, rate=rates)
    assert np.array_equal(run_deinterleave(dec, soft, max_sym, max_sym * 216, rates=rates), want)        # counts absent: whole symbols


@pytest.mark.parametrize("rate", range(8))
def test_one_rate_for_all_frames_strides_and_one_frame(rate):
    dec = decoder("SOFT16")
    rng = np.random.default_rng(10 + rate)
    r, max_sym = WIFI_RATES[rate], 2
    for frames, width in ((1, max_sym * r.n_cbps), (5, max_sym * r.n_cbps), (300, max_sym * r.n_cbps + 3)):
        soft = soft_bits(rng, np.int16, (frames, width))
        S = max_sym * r.n_dbps
        want = wifi_deinterleave_numpy(soft, max_sym, S, rate=rate)
        assert np.array_equal(run_deinterleave(dec, soft, max_sym, S, rate=rate, stride=width), want)
        n_steps = rng.integers(0, S + 3, size=frames).tolist()
        want = wifi_deinterleave_numpy(soft, max_sym, S + 6, rate=rate, n_steps=n_steps)
        assert np.array_equal(run_deinterleave(dec, soft, max_sym, S + 6, rate=rate, n_steps=n_steps, stride=width), want)
    import torch
    d = torch.from_numpy(soft).cuda()
    view = d[:, :max_sym * r.n_cbps]                               # the Python layer reads a view with its row stride
    assert np.array_equal(dec.wifi_deinterleave(view, max_sym, S, rate=rate).cpu().numpy(), wifi_deinterleave_numpy(soft, max_sym, S, rate=rate))


def test_length_4095_at_6_mbit():
    """the largest indices: 1366 OFDM symbols in one frame"""
    dec = decoder("SOFT16")
    n_steps = 16 + 8 * 4095 + 6
    max_sym = -(-n_steps // 24)
    assert max_sym == 1366
    soft = soft_bits(np.random.default_rng(2), np.int16, (1, max_sym * 48))
    S = max_sym * 24
    want = wifi_deinterleave_numpy(soft, max_sym, S, rate=0, n_steps=[n_steps])
    got = run_deinterleave(dec, soft, max_sym, S, rate=0, n_steps=[n_steps], stride=max_sym * 48)
    assert np.array_equal(got, want) and got[0, n_steps - 1].all() and not got[0, n_steps:].any()


def test_one_frame_through_the_python_layer_with_the_output_right_behind_the_input():
    """one frame's row is narrower than the ABI's default stride of max_sym * 288: the Python layer passes the row's own width, so an
    output that starts where the row ends is not taken for an overlap"""
    import torch
    dec = decoder("SOFT16")
    rng = np.random.default_rng(21)
    for rate, max_sym in ((0, 1), (0, 3), (1, 2), (3, 2), (5, 1), (7, 2)):
        r = WIFI_RATES[rate]
        n, S = max_sym * r.n_cbps, max_sym * r.n_dbps
        soft = soft_bits(rng, np.int16, (1, n))
        arena = torch.full((n + 2 * S + GUARD,), FILL16, dtype=torch.int16, device="cuda")
        arena[:n] = torch.from_numpy(soft[0]).cuda()
        want = wifi_deinterleave_numpy(soft, max_sym, S, rate=rate)
        for row in (arena[:n].view(1, n), arena[:n]):                                   # [1][n] and one frame [n]
            arena[n:] = FILL16
            got = dec.wifi_deinterleave(row, max_sym, S, rate=rate, out=arena[n:n + 2 * S].view(1, S, 2))
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), want) and (arena[n + 2 * S:] == FILL16).all()
            assert np.array_equal(arena[:n].cpu().numpy(), soft[0])
    # the SIGNAL stage of WifiDecoder on ONE PPDU, its symbol buffer placed right behind the soft bits, then the whole chain
    spec = [(0, 9, 77)]
    signal_soft, data_soft, psdus = cases.make_ppdus(spec, 4, seed=5)
    image, status, signal = cases.cpu_chain(signal_soft, data_soft, 4)
    assert status[0].tolist() == [9, 77, 0, 0]
    wifi = WifiDecoder(dec, dec, 4)
    arena = torch.zeros(48 + 48, dtype=torch.int16, device="cuda")
    arena[:48] = torch.from_numpy(signal_soft[0]).cuda()
    wifi._buffers(1)
    wifi._sig_sym = arena[48:].view(1, 24, 2)                      # where an allocator may put it: the 96 bytes behind the 96 of the input
    psdu, st, sig = wifi.decode(arena[:48].view(1, 48), torch.from_numpy(data_soft.copy()).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(sig.cpu().numpy().view(np.uint32), signal) and np.array_equal(st.cpu().numpy().view(np.uint32), status)
    assert psdu.cpu().numpy()[0, :9].tobytes() == psdus[0].tobytes()


def test_the_signal_parser():
    import torch
    dec = decoder("SOFT16")
    rng = np.random.default_rng(3)
    for frames, stride in ((1, 3), (700, 3), (33, 5)):
        fields = rng.integers(0, 256, size=(frames, stride), dtype=np.uint8)
        fields[::3, 0] = (fields[::3, 0] & 0x07) | rng.choice([0xD0, 0xF0, 0x50, 0x70, 0x90, 0xB0, 0x10, 0x30], size=fields[::3].shape[0])
        want = wifi_signal_parse_numpy(fields)
        d = torch.from_numpy(fields).cuda()
        out = torch.full((frames * 5 + GUARD,), -1, dtype=torch.int32, device="cuda")
        got = dec.wifi_signal_parse(d, out=out[:frames * 5].view(frames, 5))
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want) and (out[frames * 5:] == -1).all()
        assert np.array_equal(d.cpu().numpy(), fields)
        if frames > 1:
            assert 0 < want[:, 4].sum() < frames


def data_field(rng, S, psdu, seed):
    """the decoded bytes of a DATA field of S steps that carries `psdu`, scrambled from `seed`; random pad"""
    n_bits = S - 6
    bits = rng.integers(0, 2, size=n_bits, dtype=np.uint8)
    bits[:16] = 0
    bits[16:16 + 8 * len(psdu)] = np.unpackbits(np.asarray(psdu, dtype=np.uint8), bitorder="little")
    return np.packbits(bits ^ wifi_scrambler_numpy(seed, n_bits))


def run_descramble(dec, data, S, lengths, max_length, length_stride=1, psdu_stride=0):
    """the call through the C ABI -> (psdu image [frames][stride] over the fill, status uint32 [frames][4]), guards checked"""
    import torch
    frames = data.shape[0]
    d_in = torch.from_numpy(data.copy()).cuda()
    ps = psdu_stride or max_length
    d_psdu = torch.full((frames * ps + GUARD,), FILL8, dtype=torch.uint8, device="cuda")
    d_status = torch.full((frames * 4 + GUARD,), -1, dtype=torch.int32, device="cuda")
    d_len = u32(lengths, length_stride)
    rc = _lib.load().vit_hip_wifi_data_batch(dec._handle._h, ptr(d_in), data.shape[1], frames, S, ptr(d_len), length_stride, max_length,
                                             ptr(d_psdu), psdu_stride, ptr(d_status), None)
    assert rc == _lib.OK, _lib.load().vit_hip_last_error()
    torch.cuda.synchronize()
    psdu, status = d_psdu.cpu().numpy(), d_status.cpu().numpy()
    assert (psdu[frames * ps:] == FILL8).all() and (status[frames * 4:] == -1).all() and np.array_equal(d_in.cpu().numpy(), data)
    return psdu[:frames * ps].reshape(frames, ps), status[:frames * 4].view(np.uint32).reshape(frames, 4)


def check_descramble(dec, data, S, lengths, max_length, **kw):
    got_psdu, got_status = run_descramble(dec, data, S, lengths, max_length, **kw)
    octets, status = wifi_descramble_numpy(data, S, np.asarray(lengths, dtype=np.uint64).astype(np.int64), max_length)
    want = np.full(got_psdu.shape, FILL8, dtype=np.uint8)
    for f, o in enumerate(octets):
        want[f, :o.size] = o
    assert np.array_equal(got_status, status), (got_status.tolist(), status.tolist())
    assert np.array_equal(got_psdu, want)
    return status


def test_the_descrambler_at_the_lengths():
    dec = decoder("SOFT16")
    rng = np.random.default_rng(4)
    lengths = [0, 3, 4, 5, 63, 64, 65, 4095, 65, 100, 64]
    S = 22 + 8 * 4095 + 5
    rows = []
    for f, n in enumerate(lengths):
        body = rng.integers(0, 256, size=max(n - 4, 0) if n >= 4 else n, dtype=np.uint8)
        psdu = cases.with_fcs(body.tobytes()) if n >= 4 else body
        rows.append(data_field(rng, S, psdu, 1 + 11 * f))
    data = np.stack(rows)
    data[9, 30] ^= 0x10                                            # a corrupted FCS' frame: one bit of the body
    data[10, 0] &= 1                                               # seven zero bits in front
    data = np.concatenate([data, rng.integers(0, 256, size=(len(lengths), 3), dtype=np.uint8)], axis=1)      # a stride above the bytes
    status = check_descramble(dec, data, S, lengths, 4095)
    good = [f for f, n in enumerate(lengths) if n >= 4 and f not in (9, 10)]
    assert (status[good, 3] == 0).all() and (status[good, 2] == 0).all() and status[good, 1].tolist() == [1 + 11 * f for f in good]
    assert status[9, 3] not in (0, 0xFFFFFFFF) and status[10, 1] == 0 and status[:2, 3].tolist() == [0xFFFFFFFF] * 2
    check_descramble(dec, data, S, lengths, 4095, length_stride=5, psdu_stride=4099)
    check_descramble(dec, data, S, lengths, 64)                   # cut at max_length: 65 and 4095 become 64 and no longer check
    # lengths above what the frame holds: S leaves room for 70 octets and a few bits
    S2 = 22 + 8 * 70 + 3
    small = rng.integers(0, 256, size=(130, (S2 - 6 + 7) // 8), dtype=np.uint8)
    hostile = [70, 71, 4095, 2 ** 32 - 1, 69, 0] + rng.integers(0, 80, size=124).tolist()
    status = check_descramble(dec, small, S2, hostile, 4095, psdu_stride=70)
    assert status[:4, 0].tolist() == [70] * 4
    check_descramble(dec, small[:1], S2, hostile[:1], 4095, psdu_stride=70)            # one frame
    check_descramble(dec, small[:, :3], 22 + 7, [0, 1, 5] * 43 + [9], 4095)            # no room for an octet: only the status is written


def test_rejections():
    import torch
    dec, lte = decoder("SOFT16"), decoder("SOFT16", 3)
    lib = _lib.load()
    d_in = torch.zeros(4 * 288, dtype=torch.int16, device="cuda")
    out = torch.full((4 * 216 * 2 + 8,), FILL16, dtype=torch.int16, device="cuda")
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")

    def deint(h=dec._handle._h, src=d_in, stride=0, frames=4, max_sym=1, rate=0, d_rate=None, S=216, dst=out, off=0, cs=0):
        return lib.vit_hip_wifi_deinterleave_batch(h, ptr(src), stride, frames, max_sym, rate, ptr(d_rate), None, None, cs, S, ptr(dst, off), None)

    assert deint() == _lib.OK and deint(frames=0, max_sym=0, S=0) == _lib.OK
    for bad in (dict(h=None), dict(src=None), dict(dst=None), dict(h=lte._handle._h), dict(rate=8), dict(max_sym=0), dict(S=0), dict(stride=47),
                dict(d_rate=counts, stride=287), dict(off=2), dict(dst=d_in), dict(d_rate=out), dict(max_sym=2 ** 32 // 288 + 1),
                dict(S=2 ** 31 - 1), dict(frames=2 ** 33, S=1)):
        assert deint(**bad) == _lib.ERR_INVALID_ARG, bad
    assert deint(rate=8, d_rate=counts) == _lib.OK                 # with d_rate the scalar is not looked at
    torch.cuda.synchronize()
    assert (out[4 * 216 * 2:] == FILL16).all()

    b = torch.zeros(4 * 40, dtype=torch.uint8, device="cuda")
    sig = torch.zeros(4 * 5 + 1, dtype=torch.int32, device="cuda")
    assert lib.vit_hip_wifi_signal_batch(dec._handle._h, ptr(b), 0, 4, ptr(sig), None) == _lib.OK
    for args in ((None, ptr(b), 0, 4, ptr(sig)), (dec._handle._h, None, 0, 4, ptr(sig)), (dec._handle._h, ptr(b), 0, 4, None),
                 (dec._handle._h, ptr(b), 2, 4, ptr(sig)), (dec._handle._h, ptr(b), 0, 4, ptr(sig, 2)), (dec._handle._h, ptr(sig), 0, 4, ptr(sig))):
        assert lib.vit_hip_wifi_signal_batch(*args, None) == _lib.ERR_INVALID_ARG
    assert lib.vit_hip_wifi_signal_batch(dec._handle._h, ptr(b), 0, 0, ptr(sig), None) == _lib.OK

    psdu = torch.full((4 * 16,), FILL8, dtype=torch.uint8, device="cuda")
    status = torch.full((4 * 4,), -1, dtype=torch.int32, device="cuda")

    def data(h=dec._handle._h, src=b, stride=0, frames=4, S=22 + 8 * 16, lengths=counts, ls=0, max_length=16, dst=psdu, ps=0, st=status, st_off=0):
        return lib.vit_hip_wifi_data_batch(h, ptr(src), stride, frames, S, ptr(lengths), ls, max_length, ptr(dst), ps, ptr(st, st_off), None)

    assert data() == _lib.OK and data(frames=0) == _lib.OK
    for bad in (dict(h=None), dict(src=None), dict(lengths=None), dict(dst=None), dict(st=None), dict(S=21), dict(S=2 ** 31 - 1), dict(stride=17),
                dict(ps=15), dict(st_off=2), dict(dst=b), dict(st=counts), dict(max_length=2 ** 28)):
        assert data(**bad) == _lib.ERR_INVALID_ARG, bad
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        lte.wifi_deinterleave(d_in.view(4, 288), 1, 24)
    with pytest.raises(ValueError):
        dec.wifi_deinterleave(d_in.view(4, 288), 7, 24)            # seven symbols at 6 Mbit/s need 336
    with pytest.raises(ValueError):
        dec.wifi_signal_parse(b.view(4, 40)[:, :2])
    with pytest.raises(ValueError):
        dec.wifi_descramble(b.view(4, 40), 22 + 8 * 40, counts[:4])


# 64 PPDUs of mixed rate and length; the scrambler seeds differ.  sigma = 0.2 of the amplitude is 14 dB: far inside what the rate 3/4
# code at 54 Mbit/s corrects, so that the CPU composition recovers every frame -- which the test asserts of its input
CHAIN_MAX_SYM = 6
CHAIN_SPECS = [(f % 8, 4 + (37 * f) % (cases.largest_length(f % 8, CHAIN_MAX_SYM) - 3), 1 + (29 * f) % 127) for f in range(64)]


@functools.lru_cache(maxsize=None)
def chain_case(seed):
    signal_soft, data_soft, psdus = cases.make_ppdus(CHAIN_SPECS, CHAIN_MAX_SYM, seed=seed, sigma=0.2)
    image, status, signal = cases.cpu_chain(signal_soft, data_soft, CHAIN_MAX_SYM)
    # a condition on the input, checked on the CPU side: the CPU composition alone recovers every frame
    assert (signal[:, 4] == 1).all() and (status[:, 3] == 0).all() and (status[:, 2] == 0).all()
    assert status[:, 0].tolist() == [s[1] for s in CHAIN_SPECS] and signal[:, 0].tolist() == [s[0] for s in CHAIN_SPECS]
    for f, p in enumerate(psdus):
        assert image[f, :p.size].tobytes() == p.tobytes()
    for x in (signal_soft, data_soft, image, status, signal):
        x.setflags(write=False)
    return signal_soft, data_soft, image, status, signal


def test_the_whole_chain_on_64_ppdus():
    import torch
    signal_soft, data_soft, image, status, signal = chain_case(7)
    assert (np.abs(data_soft) < 127).mean() > 0.3                  # the noise is there
    wifi = WifiDecoder(decoder("SOFT16"), decoder("SOFT16"), CHAIN_MAX_SYM)
    assert wifi.max_length == image.shape[1]
    out = (torch.full(image.shape, cases.FILL, dtype=torch.uint8, device="cuda"), torch.full((64, 4), -1, dtype=torch.int32, device="cuda"),
           torch.full((64, 5), -1, dtype=torch.int32, device="cuda"))
    psdu, st, sig = wifi.decode(torch.from_numpy(signal_soft.copy()).cuda(), torch.from_numpy(data_soft.copy()).cuda(), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(sig.cpu().numpy().view(np.uint32), signal)
    assert np.array_equal(st.cpu().numpy().view(np.uint32), status)
    assert np.array_equal(psdu.cpu().numpy(), image)


@functools.lru_cache(maxsize=None)
def side_stream():
    """the one stream the graph tests of the 802.11a/g route warm up on: created once, so that they take one stream from torch's pool"""
    import torch
    return torch.cuda.Stream()


def test_the_chain_captured_into_a_graph():
    import torch
    wifi = WifiDecoder(decoder("SOFT16"), decoder("SOFT16"), CHAIN_MAX_SYM)
    first = chain_case(7)
    d_signal, d_data = torch.from_numpy(first[0].copy()).cuda(), torch.from_numpy(first[1].copy()).cuda()
    out = (torch.empty(first[2].shape, dtype=torch.uint8, device="cuda"), torch.empty((64, 4), dtype=torch.int32, device="cuda"),
           torch.empty((64, 5), dtype=torch.int32, device="cuda"))
    side = side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wifi.decode(d_signal, d_data, out=out)                     # warm-up outside the capture: every buffer is allocated here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wifi.decode(d_signal, d_data, out=out)
    for seed in (8, 7):
        signal_soft, data_soft, image, status, signal = chain_case(seed)
        d_signal.copy_(torch.from_numpy(signal_soft.copy()).cuda()), d_data.copy_(torch.from_numpy(data_soft.copy()).cuda())
        out[0].fill_(cases.FILL), out[1].fill_(-1), out[2].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[2].cpu().numpy().view(np.uint32), signal)
        assert np.array_equal(out[1].cpu().numpy().view(np.uint32), status)
        assert np.array_equal(out[0].cpu().numpy(), image)
