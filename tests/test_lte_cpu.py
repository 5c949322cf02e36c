"""viterbidecodercpp_amd/lte.py against the literal restatement of tests/lte_reference.py: the rate-matching map at every D in 1 .. 300 and
at 1024 and 8192, the hand-checked values of D = 32 and 33, match followed by de-match, the host rule against the scalar loop, the Gold
sequence, the PDCCH candidates; and the kernel's own source run on the host under the address and undefined-behaviour sanitizers
(tests/cpp/lte_host_check.cpp).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import (LTE_CC_COLUMN_PERMUTATION, lte_gold_sequence, lte_rate_dematch_numpy, lte_rate_match_map,
                                   lte_rate_match_numpy, pdcch_candidates)
from tests import lte_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D33 = [2, 18, 10, 26, 6, 22, 14, 30, 4, 20, 12, 28, 8, 24, 16, 0, 32, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31]


def test_the_map_equals_the_literal_interleaver_at_every_length():
    assert list(LTE_CC_COLUMN_PERMUTATION) == ref.PATTERN and sorted(ref.PATTERN) == list(range(32))
    for D in list(range(1, 301)) + [1024, 8192]:
        got = lte_rate_match_map(D)
        assert got.dtype == np.int32 and got.tolist() == ref.rate_match_map(D), D
        assert sorted(got.tolist()) == list(range(3 * D))


def test_the_hand_checked_values():
    m32, m33 = lte_rate_match_map(32), lte_rate_match_map(33)
    for i in range(3):
        assert m32[32 * i:32 * (i + 1)].tolist() == [3 * d + i for d in ref.PATTERN]
        assert m33[33 * i:33 * (i + 1)].tolist() == [3 * d + i for d in D33]
    assert [q // 3 for q in ref.rate_match_map(33)[:33]] == D33


@pytest.mark.parametrize("D,E", [(1, 1), (7, 20), (32, 96), (33, 100), (40, 1920), (43, 72), (43, 144), (43, 576), (70, 425)])
def test_match_then_dematch_counts_the_repetitions(D, E):
    rng = np.random.default_rng(D * 1000 + E)
    coded = (1 - 2 * rng.integers(0, 2, size=(3, D, 3))).astype(np.int16)
    sent = lte_rate_match_numpy(coded, E)
    assert sent.shape == (3, E) and sent.flags.c_contiguous and sent[1].tolist() == ref.rate_match(coded[1].reshape(-1).tolist(), E)
    back = lte_rate_dematch_numpy(sent.reshape(-1), 3, D, E, received_frame_stride=E)
    where = lte_rate_match_map(D)
    times = np.zeros(3 * D, dtype=np.int64)
    np.add.at(times, where[np.arange(E) % (3 * D)], 1)
    assert times.sum() == E and times.max() - times.min() <= 1
    assert (E >= 3 * D) == bool(times.min() > 0)
    assert np.array_equal(back.reshape(3, -1), coded.reshape(3, -1) * times)


def test_the_host_rule_equals_the_scalar_loop():
    rng = np.random.default_rng(5)
    for dtype, full in ((np.int16, 32767), (np.int8, 127)):
        for D, E_max, shift in ((1, 7, 0), (31, 100, 1), (33, 99, 0), (40, 1920, 4), (43, 576, 2), (65, 400, 0)):
            n = 3000
            received = rng.integers(-full - 1, full + 1, size=n).astype(dtype)
            received[:200] = -full - 1                                            # the negation of the lowest value, many times over
            offsets = np.array([0, 1, 77, n - 5, n, n + 9, 2 ** 32 - 1, 300], dtype=np.uint32)
            counts = np.array([E_max, 0, 5, E_max + 7, 3, 3, 3, 2 ** 32 - 1], dtype=np.uint32)
            bits = rng.integers(0, 2, size=n).tolist()
            for period in (0, 64, E_max):
                want = ref.dematch(received.tolist(), 8, D, E_max, offsets=offsets, counts=counts, mask_bits=bits, period=period, shift=shift,
                                   lo=-full + 3, hi=full - 1)
                got = lte_rate_dematch_numpy(received, 8, D, E_max, offsets=offsets, counts=counts, scramble=ref.pack_bits(bits),
                                             scramble_period=period, shift=shift, clamp_lo=-full + 3, clamp_hi=full - 1)
                assert got.dtype == dtype and got.shape == (8, D, 3) and got.reshape(-1).tolist() == want, (dtype, D, period)
            frames = n // E_max
            want = ref.dematch(received.tolist(), min(frames, 3), D, E_max, stride=E_max, shift=shift, lo=-full - 1, hi=full)
            got = lte_rate_dematch_numpy(received, min(frames, 3), D, E_max, received_frame_stride=E_max, shift=shift, clamp_lo=-full - 1, clamp_hi=full)
            assert got.reshape(-1).tolist() == want
    with pytest.raises(ValueError):
        lte_rate_dematch_numpy(np.zeros(10, dtype=np.int16), 2, 3, 6, received_frame_stride=6)
    with pytest.raises(ValueError):
        lte_rate_dematch_numpy(np.zeros(10, dtype=np.int32), 1, 3, 6, received_frame_stride=6)


def test_the_int32_sum_wraps():
    received = np.full(200001, 32767, dtype=np.int16)             # D = 1: 66667 repetitions of each of the three outputs
    want = ref.dematch(received.tolist(), 1, 1, 200001, stride=200001, shift=0, lo=-32768, hi=32767)
    got = lte_rate_dematch_numpy(received, 1, 1, 200001, received_frame_stride=200001)
    assert got.reshape(-1).tolist() == want == [-32768] * 3 and ref.wrap32(66667 * 32767) < 0


@pytest.mark.parametrize("c_init", [0, 1, 2 ** 31 - 1, 301])
def test_the_gold_sequence(c_init):
    packed, bits = lte_gold_sequence(c_init, 1925)
    want = ref.gold_bits(c_init, 1925)
    assert bits.dtype == np.uint8 and bits.tolist() == want
    assert packed.dtype == np.uint8 and np.array_equal(packed, ref.pack_bits(want)) and len(packed) == 241
    if c_init == 0:                                                # x1 alone: the recurrence from x1(0) = 1, read from 1600 on
        x1 = [1] + [0] * 30
        for i in range(1600 + 1925):
            x1.append(x1[i + 3] ^ x1[i])
        assert want == x1[1600:1600 + 1925]
    assert lte_gold_sequence(c_init, 0)[1].size == 0
    with pytest.raises(ValueError):
        lte_gold_sequence(2 ** 31, 8)


def test_pdcch_candidates():
    offsets, counts = pdcch_candidates(10)
    assert offsets.dtype == counts.dtype == np.uint32
    assert counts.tolist() == [72] * 10 + [144] * 5 + [288] * 2 + [576]
    assert offsets.tolist() == [72 * m for m in range(10)] + [144 * m for m in range(5)] + [0, 288] + [0]
    assert (offsets.astype(np.int64) + counts <= 720).all() and (offsets % counts == 0).all()
    offsets, counts = pdcch_candidates(8, levels=(4, 8))
    assert offsets.tolist() == [0, 288, 0] and counts.tolist() == [288, 288, 576]
    assert pdcch_candidates(0)[0].size == 0


def test_the_kernel_source_on_the_host_under_the_sanitizers(tmp_path):
    """tests/cpp/lte_host_check.cpp: the kernel's device functions compiled by g++ with the HIP built-ins stubbed, as a program of its own
    -- with the address and undefined-behaviour sanitizers where g++ links them --, run as a child process: the closed form of the
    position at every D, and random shapes whose buffers end their heap blocks against a literal restatement.  In front of the shapes the
    program walks the argument rule: an accepted call, every INVALID_ARG case of tests/test_gpu_lte_dematch.py, the zero-work cases.  Only
    where the linker reports that it cannot find a sanitizer's runtime is the program built without them, and the test prints which build ran"""
    exe = str(tmp_path / "lte_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "lte_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("lte_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "400", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 400 shapes"), q.stdout
