"""BatchDecoder.dvbt_deinterleave (vit_hip_dvbt_deinterleave_batch) on the GPU against the numpy rule of viterbidecodercpp_amd.dvbt and the
independent restatement of tests/dvbt_reference.py, on every byte of the output buffer from a 0x5A fill, the guard region behind each
row included: all 3 modes x v in {2, 4, 6} x 5 rates, both first parities, both symbol widths, n_sym in {1, 2, 3}, rows in {1, 3} at an
input stride and an output pitch of their own; the parity counters across two calls and in a captured graph replayed twice; every
rejected argument with a live handle; and the whole chain from transport packets to DvbtDecoder.take_frames(), noise-free and in white
Gaussian noise at an SNR at which the chain by the host rules, run on the CPU first, recovers every packet.  The transmit side and the
host chain are in tests/dvbt_cases.py.  tests/test_gpu_dvbt_edges.py goes on from here: every remainder of the workgroup remap with up
to 67 rows, a frame of 68 symbols, HARD8, each counter array alone, and DvbtDecoder with lockstep streams, parity=1, the cuts, 4k and 8k,
16-QAM, 2/3 and 5/6, 8-bit symbols and its rejections."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, DVBT_MODES, BatchDecoder, _lib, dvbt_deinterleave_numpy, dvbt_steps_per_symbol
from tests import dvbt_reference as ref
from tests.dvbt_cases import NOISE_SEED, SNR_DB, host_chain, receive, transmit
from tests.helpers import make_table_config

pytestmark = pytest.mark.gpu

FILL = 0x5A
ALL = [(m, v, r) for m in ("2k", "4k", "8k") for v in (2, 4, 6) for r in range(5)]


@functools.lru_cache(maxsize=None)
def decoder(decode_type="SOFT16"):
    code = COMMON_CODES[2]
    pc, table, config = make_table_config(code, decode_type)
    return code, pc, BatchDecoder(table, config)


def filled(dec, shape):
    import torch
    n = int(np.prod(shape)) * dec._soft_dtype.itemsize
    return torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dec._soft_dtype).view(*shape)


def run(dec, pc, mode, v, rate, rows, n_sym, first, seed, guard=3, in_guard=5, counters=True):
    """one call on random symbols in rows of their own stride, into a pitch of n_sym * steps + guard (even at 8-bit symbols): the output
    image and the image the numpy rule predicts, every byte; the reference must agree with the rule"""
    import torch
    rng = np.random.default_rng(seed)
    cell, steps = DVBT_MODES[mode].n_max * v, n_sym * dvbt_steps_per_symbol(mode, v, rate)
    info = np.iinfo(pc.soft_dtype)
    x = rng.integers(info.min, info.max + 1, size=(rows, n_sym, cell), dtype=np.int64).astype(pc.soft_dtype)
    x[x == 0] = 1                                                   # 0 is the erasure: a kept value never looks like one
    d_in = filled(dec, (rows, n_sym * cell + in_guard))
    d_in[:, :n_sym * cell] = torch.from_numpy(x.reshape(rows, -1)).cuda()
    d_out = filled(dec, (rows, steps + guard, 2))
    first = np.broadcast_to(np.asarray(first, dtype=np.int64), (rows,))
    if counters:
        p_in = torch.tensor(first.astype(np.uint32).view(np.int32).tolist(), dtype=torch.int32, device="cuda")
        p_out = torch.full((rows,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        parity = (p_in, p_out)
    else:
        parity = int(first[0])
    view = d_in[:, :n_sym * cell].view(rows, n_sym, cell)
    got = dec.dvbt_deinterleave(view if rows > 1 else view[0], mode, v, rate, parity=parity, out=d_out if rows > 1 else d_out[0])
    torch.cuda.synchronize()
    assert got.data_ptr() == d_out.data_ptr()
    if counters:
        assert np.array_equal(p_out.cpu().numpy().view(np.uint32), (first + n_sym).astype(np.uint32))
        assert np.array_equal(p_in.cpu().numpy().view(np.uint32), first.astype(np.uint32))
    want = np.frombuffer(bytes([FILL]) * (rows * (steps + guard) * 2 * x.itemsize), dtype=pc.soft_dtype).reshape(rows, steps + guard, 2).copy()
    want[:, :steps] = dvbt_deinterleave_numpy(x, mode, v, rate, first & 1)
    assert np.array_equal(want[:, :steps], ref.deinterleave(x, mode, v, rate, first & 1))
    return d_out.cpu().numpy(), want


@pytest.mark.parametrize("mode,v,rate", ALL, ids=["-".join(map(str, c)) for c in ALL])
def test_every_mode_constellation_and_rate(mode, v, rate):
    case = ALL.index((mode, v, rate))
    for decode_type, guard in (("SOFT16", 3), ("SOFT8", 4)):
        _, pc, dec = decoder(decode_type)
        # one row: n_sym 1 or 3 by turns, the scalar parity 0 or 1 by turns; three rows of two symbols with counters of both parities
        got, want = run(dec, pc, mode, v, rate, 1, 1 + 2 * (case % 2), (case // 2) % 2, case, guard, counters=False)
        assert np.array_equal(got, want)
        got, want = run(dec, pc, mode, v, rate, 1, 2, 1 - (case // 2) % 2, case + 100, guard, counters=False)
        assert np.array_equal(got, want)
        got, want = run(dec, pc, mode, v, rate, 3, 2 + case % 2, [4, 7, 0xFFFFFFFF], case + 200, guard)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_the_counter_across_two_calls_equals_one_call(decode_type):
    import torch
    _, pc, dec = decoder(decode_type)
    mode, v, rate, rows = "2k", 4, 2, 2
    cell, sps = 1512 * v, dvbt_steps_per_symbol(mode, v, rate)
    rng = np.random.default_rng(5)
    x = rng.integers(1, 100, size=(rows, 4, cell)).astype(pc.soft_dtype)
    d = torch.from_numpy(x).cuda()
    a = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    b, c = torch.zeros_like(a), torch.zeros_like(a)
    whole = dec.dvbt_deinterleave(d, mode, v, rate, parity=(a, c))
    first = dec.dvbt_deinterleave(d[:, :1], mode, v, rate, parity=(a, b))       # a view: the row stride is that of four symbols
    second = dec.dvbt_deinterleave(d[:, 1:], mode, v, rate, parity=(b, a))
    torch.cuda.synchronize()
    assert np.array_equal(torch.cat([first, second], dim=1).cpu().numpy(), whole.cpu().numpy())
    assert a.tolist() == [5, 6] and c.tolist() == [5, 6] and b.tolist() == [2, 3]
    assert np.array_equal(whole.cpu().numpy(), dvbt_deinterleave_numpy(x, mode, v, rate, [1, 0]))
    assert first.shape == (rows, sps, 2)


def test_a_captured_graph_replayed_twice_advances_parity():
    """two calls of one OFDM symbol each in one graph, the counters going a -> b -> a: a replay leaves them two further on, so every replay
    starts at the parity it would have in one long call"""
    import torch
    _, pc, dec = decoder()
    mode, v, rate = "2k", 2, 1
    cell, sps = 1512 * v, dvbt_steps_per_symbol(mode, v, rate)
    rng = np.random.default_rng(6)
    x = rng.integers(1, 100, size=(1, 6, cell)).astype(pc.soft_dtype)
    d_in = torch.zeros((1, 2, cell), dtype=dec._soft_dtype, device="cuda")
    d_out = torch.zeros((1, 2 * sps, 2), dtype=dec._soft_dtype, device="cuda")
    a = torch.tensor([1], dtype=torch.int32, device="cuda")
    b = torch.zeros_like(a)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            dec.dvbt_deinterleave(d_in[:, :1], mode, v, rate, parity=(a, b), out=d_out[:, :sps])
            dec.dvbt_deinterleave(d_in[:, 1:], mode, v, rate, parity=(b, a), out=d_out[:, sps:])
    torch.cuda.current_stream().wait_stream(stream)
    a.fill_(1)
    want = dvbt_deinterleave_numpy(x, mode, v, rate, 1)
    for replay in range(3):
        d_in.copy_(torch.from_numpy(x[:, 2 * replay:2 * replay + 2]).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want[:, 2 * replay * sps:(2 * replay + 2) * sps]), replay
        assert a.tolist() == [1 + 2 * (replay + 1)]


def test_rejected_arguments_launch_nothing():
    import torch
    _, pc, dec = decoder()
    _, _, dec8 = decoder("SOFT8")
    lib, h = _lib.load(), dec._handle._h
    d_in = torch.ones(2 * 2 * 3024 + 8, dtype=torch.int16, device="cuda")
    d_out = filled(dec, (2 * 2 * 3024 + 64,))
    par = torch.zeros(8, dtype=torch.int32, device="cuda")
    i, o, p = d_in.data_ptr(), d_out.data_ptr(), par.data_ptr()
    vp = C.c_void_p

    def call(handle=h, at_in=i, stride=0, rows=2, n_sym=2, mode=0, v=2, rate=0, parity=0, p_in=p, p_out=p + 16, at_out=o, pitch=0):
        return lib.vit_hip_dvbt_deinterleave_batch(handle, vp(at_in) if at_in else None, stride, rows, n_sym, mode, v, rate, parity,
                                                   vp(p_in) if p_in else None, vp(p_out) if p_out else None, vp(at_out) if at_out else None, pitch, None)

    bad = [dict(handle=None), dict(at_in=0), dict(at_out=0), dict(mode=3), dict(v=0), dict(v=3), dict(v=8), dict(rate=5), dict(at_in=i + 1),
           dict(at_out=o + 2), dict(p_in=p + 2), dict(p_out=p + 18), dict(stride=6047), dict(pitch=3023), dict(at_out=i + 8), dict(p_out=p),
           dict(p_out=p + 4), dict(p_in=o + 8), dict(p_out=o + 8), dict(p_out=i + 8), dict(rows=1 << 32), dict(n_sym=(1 << 32) // 3024 + 1, rows=1)]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    assert call(handle=dec8._handle._h, pitch=3025) == _lib.ERR_INVALID_ARG               # 8-bit symbols: an odd pitch under several rows
    code3 = COMMON_CODES[0] if COMMON_CODES[0].R != 2 else next(c for c in COMMON_CODES if c.R != 2)
    pc3, table3, config3 = make_table_config(code3, "SOFT16")
    assert call(handle=BatchDecoder(table3, config3)._handle._h) == _lib.ERR_INVALID_ARG and b"1/2" in lib.vit_hip_last_error()
    assert call(rows=0) == _lib.OK and call(n_sym=0) == _lib.OK                           # no work
    torch.cuda.synchronize()
    assert (d_out.view(torch.uint8) == FILL).all() and (par == 0).all()
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert par.tolist() == [0, 0, 0, 0, 2, 2, 0, 0] and (d_out[:2 * 2 * 3024] == 1).all() and (d_out[2 * 2 * 3024:].view(torch.uint8) == FILL).all()
    for kw in (dict(mode="16k"), dict(v=5), dict(rate=7)):
        with pytest.raises(ValueError):
            dec.dvbt_deinterleave(d_in[:2 * 3024].view(1, 2, 3024), **{**dict(mode="2k", v=2, rate=0), **kw})
    with pytest.raises(ValueError):
        dec.dvbt_deinterleave(d_in[:3000].view(1, 2, 1500), "2k", 2, 0)
    with pytest.raises(ValueError):
        dec.dvbt_deinterleave(d_in[:2 * 3024].view(1, 2, 3024), "2k", 2, 0, parity=(par[:1], par[:1]))
    for rows_of_out in (d_out[:3024].view(1, 1512, 2).expand(2, 1512, 2), d_out[:2 * 3024 + 2].as_strided((2, 1512, 2), (3022, 2, 1))):
        with pytest.raises(ValueError):                                                   # rows of out that share storage: stride 0, or below the row
            dec.dvbt_deinterleave(d_in[:2 * 3024].view(2, 1, 3024), "2k", 2, 0, out=rows_of_out)
    torch.cuda.synchronize()
    assert (d_out[2 * 2 * 3024:].view(torch.uint8) == FILL).all()


CHAIN = [("2k", 2, 0, [13, 14, 21]), ("2k", 2, 2, [9, 16]), ("2k", 6, 4, [3, 4])]
CHAIN_IDS = ["qpsk-1/2", "qpsk-3/4", "64qam-7/8"]


@pytest.mark.parametrize("mode,v,rate,cuts", CHAIN, ids=CHAIN_IDS)
def test_the_whole_chain_noise_free(mode, v, rate, cuts):
    """24 transport packets through the transmit side, pushed at uneven symbol counts: DvbtDecoder returns every packet behind the 11
    that fill the Forney delay lines, byte for byte"""
    _, pc, dec = decoder()
    N, H = 24, 11
    ts, soft = transmit(mode, v, rate, N, 11 + rate, pc)
    packets, status = receive(dec, mode, v, rate, soft, cuts)
    # the random bits that pad the last OFDM symbol may fill one more frame: what counts are the N - H packets that were sent
    assert len(packets) >= N - H and (status[:N - H] == 0).all() and np.array_equal(packets[:N - H], ts[:N - H])


@pytest.mark.parametrize("mode,v,rate,cuts", CHAIN, ids=CHAIN_IDS)
def test_the_whole_chain_in_noise(mode, v, rate, cuts):
    """the same packets (data seed 11 + rate) in white Gaussian noise of seed NOISE_SEED + rate at SNR_DB[rate]: soft bits of real
    magnitudes beside the 0 erasures of 3/4 and 7/8.  The chain by the host rules, run first, recovers every packet; DvbtDecoder then
    returns the same packets byte for byte, with the same pushes cut at uneven symbol counts"""
    _, pc, dec = decoder()
    N, H = 24, 11
    ts, soft = transmit(mode, v, rate, N, 11 + rate, pc, SNR_DB[rate], NOISE_SEED + rate)
    assert np.abs(soft).max() <= pc.soft_decision_high and len(np.unique(np.abs(soft))) > 64       # soft, not two levels
    hard = np.where(dvbt_deinterleave_numpy(transmit(mode, v, rate, N, 11 + rate, pc)[1], mode, v, rate, 0) > 0, 1, -1)
    noisy = dvbt_deinterleave_numpy(soft, mode, v, rate, 0)
    print(f"{mode} v{v} rate {rate}: {SNR_DB[rate]} dB, channel bit error rate {np.mean(hard[noisy != 0] * noisy[noisy != 0] < 0):.4f}")
    want, want_status = host_chain(soft, mode, v, rate, N)
    assert (want_status >= 0).all() and np.array_equal(want, ts[:N - H])
    print(f"  host chain: byte errors corrected per packet {want_status.tolist()}")
    packets, status = receive(dec, mode, v, rate, soft, cuts)
    print(f"  DvbtDecoder: byte errors corrected per packet {status[:N - H].tolist()}")
    assert len(packets) >= N - H and (status[:N - H] >= 0).all() and np.array_equal(packets[:N - H], want)

