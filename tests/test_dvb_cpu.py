"""viterbidecodercpp_amd.dvb without a GPU: the energy-dispersal sequence, the interleaver pair and both numpy rules against
tests/dvb_reference.py (per-branch FIFOs stepped byte by byte, a bit-level shift register) -- over the shapes the GPU tests use --, the
chunked calls against one call, the group-phase vote, the transport_error_indicator, and what the C ABI rejects before it needs a
device."""
import ctypes as C

import numpy as np
import pytest

from viterbidecodercpp_amd import (DVB_INTERLEAVER, _lib, conv_deinterleave_numpy, conv_interleave_numpy, dvb, dvb_derandomize_numpy, dvb_prbs,
                                   dvb_randomize_numpy)
from tests import dvb_reference as ref

SHAPES = [(12, 17, 204), (3, 2, 6), (5, 1, 10), (4, 3, 8), (3, 5, 9)]       # (4,3,8): D = 36 is no multiple of n; (3,5,9): n is odd
IDS = ["-".join(map(str, s)) for s in SHAPES]
FIRST = [0x03, 0xF6, 0x08, 0x34, 0x30, 0xB8, 0xA3, 0x93, 0xC9, 0x68, 0xB7, 0x73, 0xB3, 0x29, 0xAA, 0xF5]


def test_the_sequence():
    prbs = dvb_prbs()
    assert prbs.dtype == np.uint8 and prbs.shape == (1503,) and 8 * 188 - 1 == 1503
    assert prbs[:16].tolist() == FIRST and prbs[1502] == 0xCB
    assert prbs.tolist() == ref.sequence_bytes(1503)
    assert DVB_INTERLEAVER == (12, 17) and dvb.history_packets(12, 17, 204) == 11


@pytest.mark.parametrize("B,M,n", SHAPES, ids=IDS)
def test_interleaver_pair_delays_the_stream_by_the_longest_delay(B, M, n):
    H, D = dvb.history_packets(B, M, n), (B - 1) * M * B
    assert H == ref.history_packets(B, M, n)
    x = np.random.default_rng(n).integers(0, 256, size=(3 * H + 7, n), dtype=np.uint8)
    sent = conv_interleave_numpy(x, B, M)
    assert np.array_equal(sent, ref.interleave(x, B, M))
    out, nout, hist, fill = conv_deinterleave_numpy(sent, B, M)
    assert nout == len(x) - H and fill == H and np.array_equal(hist, sent[-H:])
    assert np.array_equal(out.reshape(-1), x.reshape(-1)[H * n - D:H * n - D + nout * n])
    if D % n == 0:
        assert np.array_equal(out, x[:nout])                       # x delayed by H packets


@pytest.mark.parametrize("B,M,n", SHAPES, ids=IDS)
def test_numpy_rule_equals_the_fifos_with_history_and_fill(B, M, n):
    H = dvb.history_packets(B, M, n)
    rng = np.random.default_rng(B * 100 + M)
    hist = rng.integers(0, 256, size=(H, n), dtype=np.uint8)
    for fill in (0, 1, min(4, H), H, H + 3):
        for nf in (0, 1, 5, 14):
            x = rng.integers(0, 256, size=(14, n), dtype=np.uint8)
            out, nout, new, keep = conv_deinterleave_numpy(x, B, M, hist, fill, nf)
            want, want_new, want_keep = ref.deinterleave(x[:nf], B, M, hist, fill)
            assert nout == len(want) == max(0, min(fill, H) + nf - H) and keep == want_keep == min(H, min(fill, H) + nf)
            assert np.array_equal(out, want) and np.array_equal(new[H - keep:], want_new[H - keep:])
    out, nout, new, keep = conv_deinterleave_numpy(x, B, M, None, 99)          # no history: the fill is not looked at
    want, want_new, want_keep = ref.deinterleave(x, B, M)
    assert np.array_equal(out, want) and keep == want_keep and np.array_equal(new, want_new)


@pytest.mark.parametrize("B,M,n", SHAPES, ids=IDS)
def test_forty_packets_in_five_calls_or_in_one(B, M, n):
    x = np.random.default_rng(5).integers(0, 256, size=(40, n), dtype=np.uint8)
    one = conv_deinterleave_numpy(x, B, M)
    hist, fill, outs, at = None, 0, [], 0
    for size in (1, 0, 10, 12, 17):
        out, nout, hist, fill = conv_deinterleave_numpy(x[at:at + size], B, M, hist, fill)
        outs.append(out)
        at += size
    assert at == 40 and np.array_equal(np.concatenate(outs), one[0]) and sum(map(len, outs)) == one[1]
    assert np.array_equal(hist, one[2]) and fill == one[3]


def test_randomizer_pair_and_the_reference():
    rng = np.random.default_rng(3)
    ts = rng.integers(0, 256, size=(19, 188), dtype=np.uint8)
    ts[:, 0] = 0x47
    for g in range(8):
        sent = dvb_randomize_numpy(ts, g)
        assert np.array_equal(sent, ref.scramble(ts, g))
        assert [int(b) for b in sent[:, 0]] == [0xB8 if (g + f) % 8 == 0 else 0x47 for f in range(19)]
        for phase in (g, None, 8, 0xFFFFFFFF):
            out, errors, nxt = dvb_derandomize_numpy(sent, phase)
            assert np.array_equal(out, ts) and not errors.any() and nxt == (g + 19) % 8
        want = ref.derandomize(sent, g)
        got = dvb_derandomize_numpy(np.pad(sent, ((0, 0), (0, 16))), g)         # 204-byte packets: the parity is not read
        assert all(np.array_equal(a, b) for a, b in zip(got[:2], want[:2])) and got[2] == want[2]


def test_the_group_phase_vote():
    rng = np.random.default_rng(11)
    for g in range(8):
        for nf in (1, 3, 8, 21):
            sync = np.array([0xB8 if (g + f) % 8 == 0 else 0x47 for f in range(nf)], dtype=np.uint8)
            noisy = sync.copy()
            noisy[rng.integers(0, nf)] ^= 0x21                                  # two wrong bits in one sync byte
            for s in (sync, noisy):
                assert dvb.dvb_phase_vote_numpy(s) == ref.vote(s.tolist())
            if nf >= 8:
                assert dvb.dvb_phase_vote_numpy(sync) == g == dvb.dvb_phase_vote_numpy(noisy)
    # a tie: three upright sync bytes fit g = 1 .. 5 alike (the head lies outside); the lowest wins
    assert dvb.dvb_phase_vote_numpy([0x47] * 3) == 1 == ref.vote([0x47] * 3)
    assert dvb.dvb_phase_vote_numpy([0xFF, 0x00]) == ref.vote([0xFF, 0x00])
    assert dvb.dvb_phase_vote_numpy([]) == 8 == ref.vote([])
    out, errors, nxt = dvb_derandomize_numpy(np.zeros((0, 188), dtype=np.uint8))
    assert out.shape == (0, 188) and errors.shape == (0,) and nxt == 0xFFFFFFFF
    assert dvb_derandomize_numpy(np.zeros((0, 188), dtype=np.uint8), 5)[2] == 5  # a known phase with no packet comes back
    # sync bytes with bit errors: counted against the byte the phase expects, and de-inverted, not forced
    x = rng.integers(0, 256, size=(9, 188), dtype=np.uint8)
    x[:, 0] = [0xB8, 0x47, 0x46, 0x47, 0xC7, 0x47, 0x47, 0x47, 0xB9]
    out, errors, nxt = dvb_derandomize_numpy(x)
    want = ref.derandomize(x)
    assert errors.tolist() == [0, 0, 1, 0, 1, 0, 0, 0, 1] == want[1].tolist() and nxt == 1 == want[2]
    assert out[:, 0].tolist() == [0x47, 0x47, 0x46, 0x47, 0xC7, 0x47, 0x47, 0x47, 0x46] and np.array_equal(out, want[0])


def test_the_transport_error_indicator():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, size=(10, 204), dtype=np.uint8)
    status = np.array([0, -1, 3, -1, 8, 0, -1, 0, 0, -1])
    plain = dvb_derandomize_numpy(x, 3)[0]
    out = dvb_derandomize_numpy(x, 3, status)[0]
    want = plain.copy()
    want[status < 0, 1] |= 0x80
    assert np.array_equal(out, want) and np.array_equal(out, ref.derandomize(x, 3, status)[0])
    assert (plain[status < 0, 1] < 0x80).any()                                  # the bit was set here, not found set
    assert np.array_equal(dvb_derandomize_numpy(x, 3, status, n_frames=4)[0], want[:4])


def test_numpy_rules_reject_bad_shapes():
    for B, M, n in ((1, 17, 204), (12, 0, 204), (12, 17, 200)):
        with pytest.raises(ValueError):
            conv_deinterleave_numpy(np.zeros((2, n), dtype=np.uint8), B, M)
    with pytest.raises(ValueError):
        dvb_derandomize_numpy(np.zeros((2, 187), dtype=np.uint8))
    with pytest.raises(ValueError):
        dvb_randomize_numpy(np.zeros((2, 204), dtype=np.uint8))


def test_abi_exports_and_rejects_a_null_handle_before_any_device():
    """every other argument error needs a handle, and a handle needs a device: tests/test_gpu_dvb.py"""
    lib = _lib.load()
    assert "vit_hip_deinterleave_batch" in _lib.EXPORTS and "vit_hip_dvb_derandomize_batch" in _lib.EXPORTS
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert lib.vit_hip_deinterleave_batch(None, p, 0, 1, 1, None, 12, 17, 204, None, None, 0, p, 0, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_dvb_derandomize_batch(None, p, 0, 188, 1, 1, None, None, None, p, 0, p, None, None) == _lib.ERR_INVALID_ARG
    kernels = _lib.list_kernels()
    assert any("deinterleave_kernel" in k for k in kernels) and any("dvb_derandomize_kernel" in k for k in kernels)
