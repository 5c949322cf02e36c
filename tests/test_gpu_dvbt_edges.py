"""The DVB-T route where tests/test_gpu_dvbt.py stops.  The kernel: every remainder mod 8 of the workgroup remap, block counts below 8 and
from 64 on, up to 67 rows with a parity counter each -- neighbours of opposite parity, 0xFFFFFFFF and 0x7FFFFFFF among them --; one
DVB-T frame of 68 symbols; HARD8 handles; each counter array alone and a scalar parity above 1, through the C ABI.  Every call is compared
on every byte of its output image from a 0x5A fill, guards behind the rows included, with the numpy rule and the independent restatement
(run() of tests/test_gpu_dvbt.py).  DvbtDecoder: lockstep streams against the sent packets and against single receivers; the same stream
under different cuts; parity=1; noise-free chains at 4k and 8k, 16-QAM, 2/3 and 5/6, SOFT16 and SOFT8, the default window and windows
that do not divide a symbol's steps; noisy chains at 2/3 and 5/6 at an SNR at which the chain by the host rules, run on the CPU first,
recovers every packet; and every rejected push or constructor argument, with a good stream decoded behind it.

A receiver's first internal call must see enough sync bytes for the marker lock to be the true one: every eighth sync byte is sent
inverted, so c packets give the true phase 8 ceil(c / 8) errors in 8 c bits, and below c = 8 one of the 1632 other phases can beat that
by chance.  Every first push here carries 16 000 steps or more: nine packets behind the first call at a window of 1024."""
import ctypes as C
import functools

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, DVBT_MODES, DVBT_RATES, BatchDecoder, DvbtDecoder, _lib, dvbt_deinterleave_numpy, dvbt_steps_per_symbol
from tests.dvbt_cases import FORNEY_DELAY, NOISE_SEED, SNR_DB, host_chain, receive_all, transmit
from tests.helpers import make_table_config
from tests.test_gpu_dvbt import FILL, decoder, filled, run

pytestmark = pytest.mark.gpu

H = FORNEY_DELAY

# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------

# (mode, rows, n_sym): blocks = rows * n_sym * Nmax / 504 = 3, 15, 21, 45, 24, 81, 165, 192, 603 at 2k; 6, 54 at 4k; 12 at 8k.  Those leave
# blocks & 7 == 2 out (3 5 7 5 0 1 5 0 3, 6 6, 4): 18 and 234 blocks at 2k close it, below and above 64
REMAP = ([("2k", r, n) for r, n in ((1, 1), (5, 1), (7, 1), (3, 5), (2, 4), (9, 3), (11, 5), (64, 1), (67, 3))] + [("4k", 1, 1), ("4k", 3, 3), ("8k", 1, 1)] +
         [("2k", 2, 3), ("2k", 13, 6)])


def blocks_of(mode, rows, n_sym):
    return rows * n_sym * (DVBT_MODES[mode].n_max // 504)


def row_counters(rows):
    """a counter per row, neighbours of opposite parity: odd in the even rows, even in the odd ones"""
    first = [0xFFFFFFFF, 4, 0x7FFFFFFF, 0x80000000]
    return (first + [2 * r + 1 - r % 2 for r in range(4, rows)])[:rows]


def test_the_remap_shapes_reach_every_remainder():
    counts = [blocks_of(*c) for c in REMAP]
    assert counts == [3, 15, 21, 45, 24, 81, 165, 192, 603, 6, 54, 12, 18, 234]
    assert {b & 7 for b in counts} == set(range(8)) and min(counts) < 8 and max(counts) >= 64
    assert {b for b in counts if b < 8} == {3, 6} and sum(b >= 64 for b in counts) == 5
    for rows in (1, 2, 5, 67):
        first = np.array(row_counters(rows))
        assert len(first) == rows and (np.diff(first & 1) != 0).all()
    assert {0xFFFFFFFF, 0x7FFFFFFF} <= set(row_counters(3))


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
@pytest.mark.parametrize("mode,rows,n_sym", REMAP, ids=[f"{m}-{r}x{n}-{blocks_of(m, r, n)}" for m, r, n in REMAP])
def test_every_remainder_of_the_remap(mode, rows, n_sym, decode_type):
    """v and rate go round with the case; every row has a counter of its own, so a unit that lands in the wrong row, symbol or unit shows
    in the bytes, and a counter written for the wrong row in run()'s check of them"""
    case = REMAP.index((mode, rows, n_sym))
    _, pc, dec = decoder(decode_type)
    got, want = run(dec, pc, mode, (2, 4, 6)[case % 3], case % 5, rows, n_sym, row_counters(rows), 300 + case, 3 if decode_type == "SOFT16" else 4)
    assert np.array_equal(got, want)


def test_one_frame_of_68_symbols():
    """a DVB-T frame: 68 symbols a row, two rows, 8k / 64-QAM / 3/4 at 8-bit symbols, 1632 blocks; run() holds the counters to first + 68"""
    _, pc, dec = decoder("SOFT8")
    got, want = run(dec, pc, "8k", 6, 2, 2, 68, [0xFFFFFFFF, 0x7FFFFFFE], 68, guard=6, in_guard=7)
    assert np.array_equal(got, want)


# what a period of k steps does NOT send, by rate index
PUNCTURED = {0: "", 1: "X2", 2: "X2 Y3", 3: "X2 Y3 X4 Y5", 4: "X2 X3 X4 Y5 X6 Y7"}


@pytest.mark.parametrize("mode,v,rate", [("2k", 4, 1), ("4k", 6, 3), ("8k", 2, 4)])
def test_hard8_handles(mode, v, rate):
    """hard decisions of +-1 in: the kept values come out +-1, the punctured places 0, as many as the pattern says and where it says"""
    import torch
    _, pc, dec = decoder("HARD8")
    assert (pc.soft_decision_low, pc.soft_decision_high) == (-1, 1) and pc.soft_dtype == np.int8
    rows, n_sym, guard = 2, 3, 4
    cell, sps, k = DVBT_MODES[mode].n_max * v, dvbt_steps_per_symbol(mode, v, rate), DVBT_RATES[rate][0]
    steps = n_sym * sps
    x = np.random.default_rng(400 + rate).choice(np.array([-1, 1], dtype=np.int8), size=(rows, n_sym, cell))
    d_out = filled(dec, (rows, steps + guard, 2))
    dec.dvbt_deinterleave(torch.from_numpy(x).cuda(), mode, v, rate, parity=1, out=d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    want = np.full((rows, steps + guard, 2), FILL, dtype=np.int8)
    want[:, :steps] = dvbt_deinterleave_numpy(x, mode, v, rate, 1)
    assert np.array_equal(got, want)
    body = got[:, :steps].reshape(-1, 2 * k)
    zero = np.zeros(2 * k, dtype=bool)
    for name in PUNCTURED[rate].split():
        zero[2 * (int(name[1]) - 1) + (name[0] == "X")] = True
    assert zero.sum() == k - 1
    assert np.array_equal(body == 0, np.broadcast_to(zero, body.shape)) and (np.abs(body[:, ~zero]) == 1).all()
    assert (got[:, :steps] == 0).sum() == rows * n_sym * (sps // k) * (k - 1) == rows * (2 * steps - n_sym * cell)


def abi(dec, d_in, rows, n_sym, mode, v, rate, parity, p_in, p_out, d_out, pitch):
    """vit_hip_dvbt_deinterleave_batch on the default stream; p_in and p_out are addresses or None"""
    import torch
    vp = C.c_void_p
    rc = _lib.load().vit_hip_dvbt_deinterleave_batch(dec._handle._h, vp(d_in.data_ptr()), 0, rows, n_sym, DVBT_MODES[mode].index, v, rate, parity,
                                                     vp(p_in) if p_in else None, vp(p_out) if p_out else None, vp(d_out.data_ptr()), pitch, None)
    torch.cuda.synchronize()
    return rc


def image(pc, x, mode, v, rate, first, guard):
    """the output image the rule predicts in a pitch of steps + guard from the fill"""
    rows, steps = x.shape[0], x.shape[1] * dvbt_steps_per_symbol(mode, v, rate)
    want = np.frombuffer(bytes([FILL]) * (rows * (steps + guard) * 2 * x.itemsize), dtype=pc.soft_dtype).reshape(rows, steps + guard, 2).copy()
    want[:, :steps] = dvbt_deinterleave_numpy(x, mode, v, rate, first)
    return want


def abi_case(decode_type, rows, n_sym, mode, v, seed):
    import torch
    _, pc, dec = decoder(decode_type)
    info = np.iinfo(pc.soft_dtype)
    x = np.random.default_rng(seed).integers(1, info.max + 1, size=(rows, n_sym, DVBT_MODES[mode].n_max * v), dtype=np.int64).astype(pc.soft_dtype)
    return pc, dec, x, torch.from_numpy(x).cuda()


SENTINELS = (0x13579BDF, 0x2468ACE0)


def counter_words(values):
    """int32 CUDA tensor: a sentinel, the values, a sentinel"""
    import torch
    words = np.array([SENTINELS[0], *values, SENTINELS[1]], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()).cuda(), words


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_the_counters_read_alone(decode_type):
    """d_parity_in with d_parity_out NULL: the rows' counters decide, the scalar -- given as either parity -- is ignored, and no word of
    the counter array or beside it changes"""
    mode, v, rate, rows, n_sym, guard = "2k", 4, 2, 5, 3, 4
    pc, dec, x, d_in = abi_case(decode_type, rows, n_sym, mode, v, 500)
    first = np.array(row_counters(rows), dtype=np.int64)
    par, words = counter_words(first)
    steps = n_sym * dvbt_steps_per_symbol(mode, v, rate)
    want = image(pc, x, mode, v, rate, first & 1, guard)
    for scalar in (0, 1):
        d_out = filled(dec, (rows, steps + guard, 2))
        assert abi(dec, d_in, rows, n_sym, mode, v, rate, scalar, par.data_ptr() + 4, None, d_out, steps + guard) == _lib.OK
        assert np.array_equal(d_out.cpu().numpy(), want), scalar
        assert np.array_equal(par.cpu().numpy().view(np.uint32), words), scalar


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_the_counters_written_alone(decode_type):
    """d_parity_out with d_parity_in NULL: every row follows the scalar and its counter becomes scalar + n_sym in 32 bits, the words
    beside the array untouched"""
    mode, v, rate, rows, n_sym, guard = "2k", 4, 2, 5, 3, 4
    pc, dec, x, d_in = abi_case(decode_type, rows, n_sym, mode, v, 501)
    steps = n_sym * dvbt_steps_per_symbol(mode, v, rate)
    for scalar in (0, 1, 0x7FFFFFFE, 0xFFFFFFFF):
        par, words = counter_words([0x5A5A5A5A] * rows)
        d_out = filled(dec, (rows, steps + guard, 2))
        assert abi(dec, d_in, rows, n_sym, mode, v, rate, scalar, None, par.data_ptr() + 4, d_out, steps + guard) == _lib.OK
        assert np.array_equal(d_out.cpu().numpy(), image(pc, x, mode, v, rate, scalar & 1, guard)), scalar
        words[1:-1] = (scalar + n_sym) & 0xFFFFFFFF
        assert np.array_equal(par.cpu().numpy().view(np.uint32), words), scalar


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
def test_only_bit_0_of_a_scalar_parity_counts(decode_type):
    mode, v, rate, rows, n_sym, guard = "4k", 2, 3, 2, 2, 2
    pc, dec, x, d_in = abi_case(decode_type, rows, n_sym, mode, v, 502)
    steps = n_sym * dvbt_steps_per_symbol(mode, v, rate)
    even, odd = image(pc, x, mode, v, rate, 0, guard), image(pc, x, mode, v, rate, 1, guard)
    assert not np.array_equal(even, odd)
    for scalar, want in ((2, even), (0xFFFFFFFF, odd), (0x80000000, even), (3, odd)):
        d_out = filled(dec, (rows, steps + guard, 2))
        assert abi(dec, d_in, rows, n_sym, mode, v, rate, scalar, None, None, d_out, steps + guard) == _lib.OK
        assert np.array_equal(d_out.cpu().numpy(), want), scalar


# ---- DvbtDecoder ------------------------------------------------------------------------------------------------------------------------------

def sent_and_clean(got, ts, n_packets, corrected=False):
    """the receiver's (packets, sync_errors, rs_status) hold the n_packets - 11 packets that were sent behind the Forney delay, in order,
    with no byte corrected (corrected=True: every codeword valid) and no sync bit wrong.  The random bits that pad the last OFDM symbol
    may fill one more frame behind them"""
    packets, sync_errors, status = got
    n = n_packets - H
    valid = (status[:n] >= 0).all() if corrected else (status[:n] == 0).all()
    return len(packets) >= n and valid and (sync_errors[:n] == 0).all() and np.array_equal(packets[:n], ts[:n])


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def lockstep(mode, v, rate, n_streams, n_packets, first_seed):
    """n_streams packet sets of seeds of their own -> (packets sent per stream, soft [n_streams][n_sym][Nmax * v])"""
    pc = decoder()[1]
    sent = [transmit(mode, v, rate, n_packets, first_seed + s, pc) for s in range(n_streams)]
    for s in sent:
        s[0].setflags(write=False)
    return [s[0] for s in sent], np.stack([s[1] for s in sent])         # shared between tests: nobody writes to them


# (mode, v, rate, n_streams, packets, cuts in symbols): 26 symbols of 1512 steps; 5 symbols of 16128 steps
LOCKSTEP = [("2k", 2, 0, 3, 24, (11, 12, 19)), ("2k", 2, 0, 1, 24, (11, 12, 19)), ("8k", 4, 1, 2, 40, (1, 3))]


@pytest.mark.parametrize("mode,v,rate,n_streams,n_packets,cuts", LOCKSTEP, ids=["2k-qpsk-1/2-x3", "2k-qpsk-1/2-x1", "8k-16qam-2/3-x2"])
def test_lockstep_streams(mode, v, rate, n_streams, n_packets, cuts):
    """streams of different packets in one receiver, pushed as views [n_streams][symbols][Nmax v] of the whole at uneven cuts: every
    stream gives its own packets, and to the byte what a single receiver gives for that row under the same cuts"""
    dec = decoder()[2]
    ts, soft = lockstep(mode, v, rate, n_streams, n_packets, 600)
    assert all(not np.array_equal(ts[0], t) for t in ts[1:])
    got = receive_all(dec, mode, v, rate, soft, cuts, n_streams=n_streams)
    assert len(got) == n_streams
    for s in range(n_streams):
        assert sent_and_clean(got[s], ts[s], n_packets), s
        assert same(got[s], receive_all(dec, mode, v, rate, soft[s], cuts)), s


def test_the_integration_example_with_four_streams():
    """INTEGRATION.md as written: DvbtDecoder(dec, "8k", v=6, rate=2) with n_streams=4 and the default window, cells int16
    [4][n_sym][6048 * 6] through push(), then finish()"""
    import torch
    dec = decoder()[2]
    ts, soft = lockstep("8k", 6, 2, 4, 60, 700)
    assert soft.shape == (4, 4, 6048 * 6) and soft.dtype == np.int16
    rx = DvbtDecoder(dec, "8k", v=6, rate=2, n_streams=4)
    cells = torch.from_numpy(soft).cuda()
    rx.push(cells[:, :3])
    first = rx.take_frames()
    rx.finish(cells[:, 3:])
    for s, (a, b) in enumerate(zip(first, rx.take_frames())):
        packets, sync_errors, rs_status = (np.concatenate([x, y]) for x, y in zip(a, b))
        assert packets.dtype == np.uint8 and packets.shape[1] == 188 and len(a[0]) > 0
        assert sent_and_clean((packets, sync_errors, rs_status.reshape(-1)), ts[s], 60), s


def test_the_cuts_do_not_show():
    """one stream of 9 symbols (2k, 16-QAM, 3/4) in one finish(), in pushes of 5, 1, 2, 1 and of 4, 3, 2 symbols: the same packets, sync
    errors and RS status.  The counter tensors change places behind odd and behind even symbol counts"""
    _, pc, dec = decoder()
    ts, soft = transmit("2k", 4, 2, 24, 800, pc)
    assert len(soft) == 9
    whole = receive_all(dec, "2k", 4, 2, soft, ())
    assert sent_and_clean(whole, ts, 24)
    for cuts in ((5, 6, 8), (4, 7)):
        assert same(whole, receive_all(dec, "2k", 4, 2, soft, cuts)), cuts


def test_a_first_symbol_of_odd_parity():
    """sent from symbol parity 1: DvbtDecoder(..., parity=1) returns every packet, at one symbol a push too.  The same soft bits under
    parity=0 give no packet that was sent: the argument is read"""
    _, pc, dec = decoder()
    ts, soft = transmit("2k", 4, 2, 24, 801, pc, parity=1)
    assert not np.array_equal(soft, transmit("2k", 4, 2, 24, 801, pc)[1])
    for cuts in ((4, 7), (4, 5, 6, 7, 8)):
        assert sent_and_clean(receive_all(dec, "2k", 4, 2, soft, cuts, parity=1), ts, 24), cuts
    packets, _, status = receive_all(dec, "2k", 4, 2, soft, (4, 7), parity=0)
    was_sent = {t.tobytes() for t in ts}
    assert not any(p.tobytes() in was_sent for p in packets) and not sent_and_clean((packets, _, status), ts, 24)


# (mode, v, rate, packets, cuts, window): steps a symbol 8064, 6048, 27216, 5040 -- none a multiple of its window
CLEAN = [("4k", 4, 1, 40, (2, 3, 6), None), ("8k", 2, 0, 40, (3, 4, 9), 1000), ("8k", 6, 2, 60, (1, 3), None), ("2k", 4, 3, 24, (4, 5), 1536)]


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8"])
@pytest.mark.parametrize("mode,v,rate,n_packets,cuts,window", CLEAN, ids=["4k-16qam-2/3", "8k-qpsk-1/2-w1000", "8k-64qam-3/4", "2k-16qam-5/6-w1536"])
def test_noise_free_chains_in_the_other_modes(mode, v, rate, n_packets, cuts, window, decode_type):
    """4k and 8k, 16-QAM, 2/3 and 5/6, at both symbol widths: transport packets through the transmit side and out of DvbtDecoder, every
    one as sent.  At SOFT16 no byte is corrected on the way.  At SOFT8 Reed-Solomon may have corrected some: the decode rule adds 8-bit
    metrics modulo 256 and errs where the encoder's input is mostly zeros, as in the start-up fill of the Forney interleaver.  The CPU
    checker's stream rule over these very symbols errs in 144 of 65 280 bits at 4k / 2/3, 228 of 97 920 at 8k /
    3/4 and 514 of 39 168 at 2k / 5/6, all in the first 16 400, and in none at 8k / 1/2.  The card gives the checker's bits
    (test_the_bits_at_8_bit_symbols_are_those_of_the_stream_rule); on it 3 of the first 29 packets at 4k / 2/3 and 4 of the first 49 at
    8k / 3/4 had one byte corrected"""
    _, pc, dec = decoder(decode_type)
    assert dvbt_steps_per_symbol(mode, v, rate) % (window or 1024) != 0
    ts, soft = transmit(mode, v, rate, n_packets, 900 + rate, None, decode_type=decode_type)
    assert soft.dtype == pc.soft_dtype and len(soft) >= 4 and set(np.unique(soft)) == {pc.soft_decision_low, pc.soft_decision_high}
    got = receive_all(dec, mode, v, rate, soft, cuts, window=window)
    n = min(len(got[0]), n_packets - H)
    print(f"{mode} v{v} rate {rate} {decode_type}: {len(got[0])} packets out, of the first {n_packets - H} as sent "
          f"{int((got[0][:n] == ts[:n]).all(axis=1).sum())}, rs_status {got[2][:n].tolist()}, sync errors {got[1][:n].tolist()}")
    assert sent_and_clean(got, ts, n_packets, corrected=decode_type == "SOFT8")


@pytest.mark.parametrize("mode,v,rate,n_packets,cuts,window", CLEAN, ids=["4k-16qam-2/3", "8k-qpsk-1/2-w1000", "8k-64qam-3/4", "2k-16qam-5/6-w1536"])
def test_the_bits_at_8_bit_symbols_are_those_of_the_stream_rule(mode, v, rate, n_packets, cuts, window, oracle):
    """what the receiver's decode emits at SOFT8, push by push, is to the bit the rule of vit_hip_decode_stream run by the CPU checker
    over dvbt_deinterleave_numpy of the whole stream: the hand-over of a symbol's steps to the window grid, at the erasure density of
    every rate.  Whether those bits are the sent ones is the decode rule's affair at 8-bit metrics, not the front end's (see the test
    above)"""
    import torch
    from tests import stream_reference as sr
    from tests.helpers import oracle_cfg
    dec = decoder("SOFT8")[2]
    ts, soft = transmit(mode, v, rate, n_packets, 900 + rate, None, decode_type="SOFT8")
    d = torch.from_numpy(soft).cuda()
    rx = DvbtDecoder(dec, mode, v, rate, window=window)
    edges = [0, *cuts, len(soft)]
    got = b"".join(rx.finish(d[a:b]) if b == len(soft) else rx.push(d[a:b]) for a, b in zip(edges[:-1], edges[1:]))
    steps = dvbt_deinterleave_numpy(soft, mode, v, rate, 0)
    want, n_bits = sr.stream_reference(oracle, COMMON_CODES[2], oracle_cfg("SOFT8", 2), steps, W=window or 1024, flags=sr.BEGIN | sr.END)
    assert rx.rx.n_bits == n_bits == len(steps) - 6 and got == want.tobytes()


# the noise seeds at which host_chain recovers every packet, found on the CPU: NOISE_SEED + rate held at both rates
NOISY = [("2k", 4, 1, (5, 6)), ("2k", 4, 3, (4, 7))]


@pytest.mark.parametrize("mode,v,rate,cuts", NOISY, ids=["16qam-2/3", "16qam-5/6"])
def test_noisy_chains_at_two_thirds_and_five_sixths(mode, v, rate, cuts):
    """24 packets (data seed 11 + rate) in white Gaussian noise of seed NOISE_SEED + rate at SNR_DB[rate]: the erasure densities the
    existing chains lack.  The chain by the host rules, run first, recovers every packet; DvbtDecoder returns the same bytes"""
    _, pc, dec = decoder()
    N = 24
    ts, soft = transmit(mode, v, rate, N, 11 + rate, pc, SNR_DB[rate], NOISE_SEED + rate)
    assert len(np.unique(np.abs(soft))) > 64
    want, want_status = host_chain(soft, mode, v, rate, N)
    assert (want_status >= 0).all() and np.array_equal(want, ts[:N - H])
    print(f"{mode} v{v} rate {rate}: {SNR_DB[rate]} dB; host chain: byte errors corrected per packet {want_status.tolist()}")
    packets, _, status = receive_all(dec, mode, v, rate, soft, cuts)
    print(f"  DvbtDecoder: byte errors corrected per packet {status[:N - H].tolist()}")
    assert len(packets) >= N - H and (status[:N - H] >= 0).all() and np.array_equal(packets[:N - H], want)


def test_rejected_pushes_leave_the_receiver_whole():
    """a push that is not whole OFDM symbols, an empty one and one of the wrong leading dimension raise ValueError before anything runs:
    in front of a stream and in the middle of it, and the stream still decodes to what was sent"""
    import torch
    _, pc, dec = decoder()
    ts, soft = lockstep("2k", 2, 0, 3, 24, 600)
    d = torch.from_numpy(soft).cuda()
    cell = 1512 * 2

    def refused(rx, bad):
        for symbols in bad:
            for call in (rx.push, rx.finish):
                with pytest.raises(ValueError):
                    call(symbols)

    rx = DvbtDecoder(dec, "2k", 2, 0)
    bad = [d[0, :2].reshape(-1)[:-2], d[0, :1, :cell - 1], d[0, :0], d[0, 0, :0], torch.zeros(0, dtype=d.dtype, device="cuda")]
    refused(rx, bad)
    rx.push(d[0, :11])
    refused(rx, bad)
    rx.finish(d[0, 11:])
    packets, sync_errors, status = rx.take_frames()
    assert sent_and_clean((packets, sync_errors, status.reshape(-1)), ts[0], 24)

    rx = DvbtDecoder(dec, "2k", 2, 0, n_streams=3)
    bad = [d[:2, :3], d[:, :0], d[:2], d[:, :1, :cell - 1], d.reshape(-1)[:-3]]                   # [2][3][cell] holds 6 = 3 x 2 symbols
    assert d[:2, :3].numel() % (3 * cell) == 0
    refused(rx, bad)
    rx.push(d[:, :11])
    refused(rx, bad)
    rx.finish(d[:, 11:])
    for s, (packets, sync_errors, status) in enumerate(rx.take_frames()):
        assert sent_and_clean((packets, sync_errors, status.reshape(-1)), ts[s], 24), s


def test_rejected_constructor_arguments():
    """a decoder that is not K = 7, R = 1/2, a bad mode, v or rate: ValueError, and a receiver made behind them works"""
    _, pc, dec = decoder()
    others = [COMMON_CODES[3], COMMON_CODES[5]]
    assert [(c.K, c.R) for c in others] == [(7, 3), (9, 2)]
    for code in others:
        _, table, config = make_table_config(code, "SOFT16")
        with pytest.raises(ValueError):
            DvbtDecoder(BatchDecoder(table, config), "2k", 2, 0)
    for kw in (dict(mode="16k"), dict(mode=2), dict(v=3), dict(v=8), dict(v=0), dict(rate=5), dict(rate=-1)):
        with pytest.raises(ValueError):
            DvbtDecoder(dec, **{**dict(mode="2k", v=2, rate=0), **kw})
        with pytest.raises(ValueError):
            DvbtDecoder(dec, **{**dict(mode="2k", v=2, rate=0, n_streams=2), **kw})
    ts, soft = lockstep("2k", 2, 0, 3, 24, 600)
    assert sent_and_clean(receive_all(dec, "2k", 2, 0, soft[1], (13,)), ts[1], 24)
