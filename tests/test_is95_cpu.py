"""viterbidecodercpp_amd/is95.py against the literal check values of include/vit_hip.h and the independent restatement of
tests/is95_reference.py: the interleaver, the combining, the rate decision with its edge cases, the two CRC codes against a bit-serial
loop, transmit -> receive round trips over the CPU oracle decoder at all four rates and both polynomial sets, noise-free and in white
Gaussian noise at the recorded seed and SNR of tests/is95_cases.py; the argument errors the ABI reports without a device; and the kernels'
own source with their argument rules run on the host as a program of its own under the address and undefined-behaviour sanitizers
(tests/cpp/is95_host_check.cpp).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, IS95_CRC8, IS95_CRC12, IS95_POLYNOMIALS, IS95_RATE_SET_1, _lib, crc_numpy, is95_deinterleave_numpy,
                                   is95_permutation, is95_rate_decide_numpy, is95_traffic_frame_numpy)
from tests import is95_cases as cases
from tests import is95_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_literal_checks_of_the_interleaver():
    a = is95_permutation()
    assert a.dtype == np.int32 and a[:8].tolist() == [0, 64, 128, 192, 256, 320, 32, 96]
    assert (a[:8] + 1).tolist() == [1, 65, 129, 193, 257, 321, 33, 97]
    assert sorted(a.tolist()) == list(range(384))                                   # a permutation
    inverse = np.empty(384, dtype=np.int64)
    inverse[a] = np.arange(384)
    bro6 = lambda x: int(format(x, "06b")[::-1], 2)
    assert inverse.tolist() == [6 * bro6(s % 64) + s // 64 for s in range(384)]
    assert (inverse[1], inverse[2], inverse[64], inverse[383]) == (192, 96, 1, 383)
    assert a.tolist() == ref.interleave(list(range(384)))                           # the array of the standard, never the formula


def test_the_frame_formats_and_the_polynomials():
    table = [(r.bps, r.repeat, r.L, r.info_bits, r.steps, r.n_bytes) for r in IS95_RATE_SET_1]
    assert table == [(9600, 1, 184, 172, 192, 23), (4800, 2, 88, 80, 96, 11), (2400, 4, 40, 40, 48, 5), (1200, 8, 16, 16, 24, 2)]
    assert [r.crc for r in IS95_RATE_SET_1] == [IS95_CRC12, IS95_CRC8, None, None]
    assert (IS95_CRC12.width, IS95_CRC12.poly, IS95_CRC12.init, IS95_CRC12.xorout) == (12, 0xF13, 0xFFF, 0)
    assert (IS95_CRC8.width, IS95_CRC8.poly, IS95_CRC8.init, IS95_CRC8.xorout) == (8, 0x9B, 0xFF, 0)
    assert all(r.steps * 2 * r.repeat == 384 and r.info_bits + (r.crc.width if r.crc else 0) == r.L for r in IS95_RATE_SET_1)
    # the stock set is 753, 561 octal read literally; the standard's reading is its bit reversal, and COMMON_CODES is as it was
    assert COMMON_CODES[5].G == (491, 369) == (0o753, 0o561) and IS95_POLYNOMIALS == (431, 285) == (0o657, 0o435)
    assert tuple(int(format(g, "09b")[::-1], 2) for g in COMMON_CODES[5].G) == IS95_POLYNOMIALS


@pytest.mark.parametrize("code", [IS95_CRC12, IS95_CRC8], ids=["crc12", "crc8"])
def test_the_crc_codes_against_a_bit_serial_loop(code):
    rng = np.random.default_rng(code.width)
    for n in (0, 1, 16, 80, 172):
        frame = rng.integers(0, 256, size=24, dtype=np.uint8)
        assert int(crc_numpy(code, frame, n)) == ref.crc_bit_serial(code.width, code.poly, code.init, np.unpackbits(frame)[:n].tolist())


@pytest.mark.parametrize("dtype", [np.int16, np.int8])
def test_the_deinterleave_rule_against_the_restatement(dtype):
    rng = np.random.default_rng(7)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max + 1, size=(6, 384)).astype(dtype)
    x[0], x[1] = info.min, info.max                                                 # both extremes: the int32 sum of eight and the clamp
    masks = rng.integers(0, 256, size=(6, 48), dtype=np.uint8)
    masks[0] = 0xFF                                                                 # -(-32768) adds as 32768
    for scramble, shift, lo, hi in ((None, 0, None, None), (masks, 0, None, None), (masks[2], 3, None, None), (masks, 3, -100, 90),
                                    (masks, 15, None, None), (masks, 0, -5, -5)):
        got = is95_deinterleave_numpy(x, scramble, shift, lo, hi)
        assert [g.shape for g in got] == [(6, 192, 2), (6, 96, 2), (6, 48, 2), (6, 24, 2)] and all(g.dtype == dtype for g in got)
        for f in range(6):
            bits = None if scramble is None else np.unpackbits(scramble if scramble.ndim == 1 else scramble[f]).tolist()
            want = ref.deinterleave(x[f].tolist(), bits, shift, info.min if lo is None else lo, info.max if hi is None else hi)
            for h in range(4):
                assert got[h][f].reshape(-1).tolist() == want[h], (f, h, shift)
    labels = np.arange(1, 385, dtype=np.int16)[None]                                # the literal checks: s[1] = y[192], s[2] = y[96], ...
    s = is95_deinterleave_numpy(labels)[0].reshape(-1)
    assert (s[1], s[2], s[64], s[383]) == (193, 97, 2, 384)
    for bad in (lambda: is95_deinterleave_numpy(np.zeros((1, 383), dtype=np.int16)), lambda: is95_deinterleave_numpy(np.zeros((1, 384), dtype=np.int32)),
                lambda: is95_deinterleave_numpy(labels, shift=16), lambda: is95_deinterleave_numpy(labels, clamp_lo=5, clamp_hi=4),
                lambda: is95_deinterleave_numpy(labels, scramble=np.zeros(47, dtype=np.uint8)), lambda: is95_traffic_frame_numpy(np.zeros(171), 0),
                lambda: is95_traffic_frame_numpy(np.zeros(16), 4)):
        with pytest.raises(ValueError):
            bad()


def _decide(present, errors, compared, syndrome, max_num, den):
    """both statements of the rule on one frame; the package's must equal the restatement's"""
    rng = np.random.default_rng(1)
    decoded = [rng.integers(0, 256, size=(1, n), dtype=np.uint8) if p else None for n, p in zip((23, 11, 5, 2), present)]
    decision, info = is95_rate_decide_numpy(decoded, [[e] for e in errors], [[c] for c in compared], [[s] for s in syndrome], max_num, den)
    want = ref.decide(present, errors, compared, syndrome, max_num, den)
    assert tuple(int(v) for v in decision[0]) == want
    bits = np.unpackbits(info[0])
    if want[0] == 4:
        assert not bits.any()
    else:
        assert bits[:want[1]].tolist() == np.unpackbits(decoded[want[0]][0])[:want[1]].tolist() and not bits[want[1]:].any()
    return want


def test_the_decision_rule_and_its_edges():
    all4, one = [True] * 4, (1, 1, 1, 1)
    assert _decide(all4, [5, 1, 9, 9], [100, 100, 100, 100], [0, 0], one, 10)[0] == 1
    assert _decide(all4, [1, 2, 4, 8], [10, 20, 40, 80], [0, 0], one, 10)[0] == 0                    # a four-way tie: the lowest h
    assert _decide(all4, [1, 2, 4, 8], [10, 20, 40, 80], [1, 0], one, 10)[0] == 1                    # ... of those that check
    assert _decide(all4, [1, 2, 4, 8], [10, 20, 40, 80], [1, 0xFFFFFFFF], one, 10)[0] == 2
    assert _decide(all4, [0, 0, 0, 0], [0, 0, 0, 7], [0, 0], one, 10) == (3, 16, 0, 7)               # compared = 0 never passes
    assert _decide(all4, [0, 0, 0, 0], [0, 0, 0, 0], [0, 0], one, 10) == (4, 0, 0, 0)
    assert _decide(all4, [11, 11, 11, 11], [100, 100, 100, 100], [0, 0], one, 10) == (4, 0, 0, 0)    # nothing under the threshold
    assert _decide(all4, [10, 11, 11, 11], [100, 100, 100, 100], [0, 0], one, 10)[0] == 0            # at the threshold passes
    assert _decide(all4, [3, 3, 3, 3], [100, 100, 100, 100], [0, 0], (0, 0, 5, 0), 100)[0] == 2      # a threshold per hypothesis
    assert _decide([False, True, False, True], [0, 9, 0, 8], [50, 100, 50, 100], [0, 0], one, 10)[0] == 3      # absent ones do not compete
    assert _decide([False, False, True, False], [0, 0, 50, 0], [50, 50, 100, 50], [0, 0], one, 10) == (4, 0, 0, 0)
    assert _decide([True, False, False, False], [7, 0, 0, 0], [384, 0, 0, 0], [0, 5], one, 10) == (0, 172, 7, 384)
    # products that need 64 bits: 3e9 / 4e9 against 2999999999 / 4e9, and a threshold product above 2^32
    big = 4000000000
    assert _decide(all4, [3000000000, 2999999999, big, big], [big] * 4, [0, 0], (3, 3, 3, 3), 4)[0] == 1
    assert _decide(all4, [3000000001, 3000000001, big, big], [big] * 4, [0, 0], (3, 3, 3, 3), 4) == (4, 0, 0, 0)
    assert _decide(all4, [65536, 65537, big, big], [big, big, big, big], [0, 0], (0xFFFFFFFF, 0xFFFFFFFF, 0, 0), 0xFFFFFFFF)[0] == 0
    rng = np.random.default_rng(2)
    for _ in range(300):                                                                              # and at random, small numbers: many ties
        present = [bool(b) for b in rng.integers(0, 2, size=4)]
        if not any(present):
            continue
        _decide(present, rng.integers(0, 6, size=4).tolist(), rng.integers(0, 12, size=4).tolist(), rng.integers(0, 2, size=2).tolist(),
                rng.integers(0, 4, size=4).tolist(), int(rng.integers(1, 6)))
    with pytest.raises(ValueError):
        is95_rate_decide_numpy([None] * 4, [[0]] * 4, [[0]] * 4, [[0]] * 2, one, 10)
    with pytest.raises(ValueError):
        is95_rate_decide_numpy([np.zeros((1, 23), dtype=np.uint8), None, None, None], [[0]] * 4, [[1]] * 4, [[0]] * 2, one, 0)


def test_byte_21_of_a_full_rate_frame_keeps_its_top_four_bits():
    decoded = [np.full((1, 23), 0xFF, dtype=np.uint8), None, None, None]
    decision, info = is95_rate_decide_numpy(decoded, [[0]] * 4, [[384]] * 4, [[0], [0]], (1, 1, 1, 1), 10)
    assert decision[0].tolist() == [0, 172, 0, 384] and info[0].tolist() == [0xFF] * 21 + [0xF0]


@pytest.mark.parametrize("name", ["stock", "standard"])
def test_round_trips_over_the_oracle_decoder_noise_free(name):
    code = cases.CODES[name]
    symbols, scramble, rates, info = cases.make_frames(code, frames=16, seed=3)
    assert sorted(rates[:4].tolist()) == [0, 1, 2, 3] and set(np.abs(symbols).reshape(-1).tolist()) == {127}
    decision, got, syndrome, counts = cases.cpu_chain(code, symbols, scramble)
    assert decision[:, 0].tolist() == rates.tolist() and np.array_equal(got, info)
    assert decision[:, 1].tolist() == [IS95_RATE_SET_1[h].info_bits for h in rates]
    assert (decision[:, 2] == 0).all() and (decision[:, 3] == 384 >> rates).all()   # no symbol differs, none is an erasure
    assert all(syndrome[h][f] == 0 for f, h in enumerate(rates) if h < 2)
    # without the masks the frames do not come back: the descrambling is part of the rule
    assert not np.array_equal(cases.cpu_chain(code, symbols, None)[1], info)


@pytest.mark.parametrize("name", ["stock", "standard"])
def test_round_trips_in_noise_at_the_recorded_seed_and_snr(name):
    """the condition the GPU test rests on: Es/N0 = 2.0 dB a received symbol, seed 95, max_ser 1/10 (tests/is95_cases.py) -- the chain by
    the host rules alone returns the sent rate, the sent info bits and a zero syndrome for every frame of the set"""
    assert (cases.NOISY_FRAMES, cases.NOISY_SEED, cases.NOISY_SNR_DB, cases.MAX_SER) == (64, 95, 2.0, ((1, 1, 1, 1), 10))
    symbols, scramble, rates, info, (decision, got, syndrome, counts) = cases.noisy_set(name)
    clean = cases.make_frames(cases.CODES[name])[0]
    raw = (np.sign(symbols) != np.sign(clean)).mean()
    assert 0.02 < raw < 0.06, raw                                                   # the decodes have work to do
    assert decision[:, 0].tolist() == rates.tolist() and np.array_equal(got, info)
    assert all(syndrome[h][f] == 0 for f, h in enumerate(rates) if h < 2)
    assert np.bincount(rates, minlength=4).tolist() == [16, 16, 16, 16]
    assert (decision[rates == 0, 2] > 0).all()                                      # every full-rate frame had symbol errors corrected


def test_the_abi_rejects_without_a_device():
    lib = _lib.load()
    for name in ("vit_hip_is95_deinterleave_batch", "vit_hip_is95_channel_errors_batch", "vit_hip_is95_rate_decide_batch"):
        assert name in _lib.EXPORTS
    buf = (C.c_uint8 * 64)(*([0x5A] * 64))
    at = C.cast(buf, C.c_void_p)
    four, sizes, nums = (C.c_void_p * 4)(at, at, at, at), (C.c_size_t * 4)(), (C.c_uint32 * 4)(1, 1, 1, 1)
    assert lib.vit_hip_is95_deinterleave_batch(None, at, 0, 1, None, 0, 0, -127, 127, four, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_is95_rate_decide_batch(None, four, sizes, four, four, four, 1, nums, 10, at, at, 0, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_is95_channel_errors_batch(None, four, four, sizes, 1, four, four, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error() and list(buf) == [0x5A] * 64
    kernels = _lib.list_kernels()
    for part in ("is95_deinterleave_kernelIs", "is95_deinterleave_kernelIa", "is95_decide_kernel", "is95_zero_kernel"):
        found = [r for name, r in kernels.items() if part in name]
        assert len(found) == 1 and found[0]["scratch_bytes"] == 0, part


def test_the_kernel_source_and_the_argument_rules_on_the_host(tmp_path):
    """tests/cpp/is95_host_check.cpp: the kernels' functions and the argument rules compiled by g++ with the HIP built-ins stubbed, as a
    program of its own with the address and undefined-behaviour sanitizers, run as a child process.  Only where the linker reports that
    it cannot find a sanitizer's runtime is the program built without them; any other failure of the sanitizer build fails the test,
    and the test prints which build ran"""
    exe = str(tmp_path / "is95_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "is95_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("is95_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "200", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 200 shapes"), q.stdout
