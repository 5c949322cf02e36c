"""viterbidecodercpp_amd/dab.py against the independent restatement of tests/dab_reference.py: the puncturing vectors and their properties,
the profile sizes, the maps, the energy-dispersal sequence, the time interleaver and de-interleaver however the frames are cut into
calls, and a FIC block through the package's CPU encoder, puncturing, depuncturing and the oracle's decode; and the kernels' own source run on the host under the address
and undefined-behaviour sanitizers (tests/cpp/dab_host_check.cpp).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, FIC_PROFILE, PI_X, DabProfile, dab_depuncture_numpy, dab_energy_dispersal_numpy, dab_prbs,
                                   dab_puncture_numpy, dab_time_deinterleave_numpy, dab_time_interleave_numpy, eep_profile,
                                   get_decoding_config, puncture_vector, synth)
from viterbidecodercpp_amd.dab import DAB_DELAYS
from tests import dab_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS_A, LEVELS_B = ("1-A", "2-A", "3-A", "4-A"), ("1-B", "2-B", "3-B", "4-B")


def test_the_puncturing_vectors():
    for i in range(1, 25):
        v = puncture_vector(i)
        assert v.dtype == bool and v.shape == (32,) and v.sum() == 8 + i and v[0::4].all()
        assert "".join("1" if x else "0" for x in v) == ref.PI[i]
        if i > 1:
            assert (v | puncture_vector(i - 1) == v).all()         # nested
    assert puncture_vector(16).tolist() == [True, True, True, False] * 8
    p15 = puncture_vector(16).copy()
    p15[30] = False
    assert puncture_vector(15).tolist() == p15.tolist()
    assert PI_X.tolist() == [True, True, False, False] * 6 and "".join(str(int(x)) for x in PI_X) == ref.TAIL
    for bad in (0, 25):
        with pytest.raises(ValueError):
            puncture_vector(bad)
    assert list(DAB_DELAYS) == [ref.delay(j) for j in range(16)] == [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_the_size_identities(n):
    for levels, info, kept in ((LEVELS_A, 192 * n, (12, 8, 6, 4)), (LEVELS_B, 768 * n, (27, 21, 18, 15))):
        for level, k in zip(levels, kept):
            p = eep_profile(level, n)
            assert p.info_bits == info and p.steps == info + 6 and p.symbols_per_frame == 4 * (info + 6)
            assert p.n_received == 64 * k * n, (level, n)
            mask = p.mask()
            assert mask.dtype == bool and mask.tolist() == [bool(x) for x in ref.mask_walk(p.segments)]
            idx, kept_symbols = ref.source_map(ref.mask_walk(p.segments))
            assert p.source_index().dtype == np.int32 and p.source_index().tolist() == idx and kept_symbols == p.n_received


def test_the_fic_profile_and_the_issue_shapes():
    assert (FIC_PROFILE.info_bits, FIC_PROFILE.n_received, FIC_PROFILE.symbols_per_frame) == (768, 2304, 3096)
    assert FIC_PROFILE.mask().tolist() == [bool(x) for x in ref.mask_walk([(21, 16), (3, 15)])]
    p = eep_profile("4-A", 1)
    assert (p.n_received, p.symbols_per_frame) == (256, 792)
    p = eep_profile("3-A", 8)
    assert (p.n_received, p.symbols_per_frame) == (3072, 6168)
    assert eep_profile("2-A", 1).segments == ((5, 13), (1, 12)) and eep_profile("2-A", 2).segments == ((1, 14), (11, 13))
    with pytest.raises(ValueError):
        eep_profile("5-A", 1)
    with pytest.raises(ValueError):
        DabProfile([(0, 3)])


def test_the_sequence():
    bits = dab_prbs(2 * 511 + 64)
    assert bits.tolist() == ref.prbs_bits(2 * 511 + 64)
    assert bits[:16].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0]
    assert np.packbits(bits[:64]).tolist() == [0x07, 0xBE, 0x2E, 0x64, 0x12, 0x9D, 0xA3, 0xCF]
    one = bits[:511]
    assert np.array_equal(bits[511:1022], one)
    assert all(not np.array_equal(np.roll(one, s), one) for s in range(1, 511))        # no shorter period
    assert int(one.sum()) == 256


@pytest.mark.parametrize("n_bits", [0, 1, 7, 8, 9, 511, 512, 768, 1022 + 3])
def test_dispersal_equals_the_shift_register_and_is_its_own_inverse(n_bits):
    rng = np.random.default_rng(n_bits)
    nb = (n_bits + 7) // 8
    x = rng.integers(0, 256, size=(3, nb + 2), dtype=np.uint8)
    got = dab_energy_dispersal_numpy(x, n_bits)
    assert got.shape == (3, nb) and got.tolist() == [ref.descramble_frame(row.tolist(), n_bits) for row in x]
    assert np.array_equal(dab_energy_dispersal_numpy(got, n_bits), x[:, :nb])
    with pytest.raises(ValueError):
        dab_energy_dispersal_numpy(x[:, :1], 9)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 100])
def test_interleave_then_deinterleave_however_the_frames_are_cut(n):
    rng = np.random.default_rng(n)
    a = rng.integers(-128, 128, size=(40, n)).astype(np.int16)
    b = dab_time_interleave_numpy(a)
    assert b.dtype == a.dtype and b.tolist() == ref.interleave(a.tolist())
    whole, nout, hist, fill = dab_time_deinterleave_numpy(b)
    assert nout == 25 and fill == 15 and np.array_equal(whole, a[:25]) and np.array_equal(hist, b[25:])
    assert whole.tolist() == ref.fifo_deinterleave(b.tolist(), n)
    for cuts in ((1, 14, 1, 24), (7, 9, 24), (16, 24), (15, 25), (40,), (1,) * 40):
        hist, fill, got, at = None, 0, [], 0
        for c in cuts:
            out, nout, hist, fill = dab_time_deinterleave_numpy(b[at:at + c], hist, fill)
            assert nout == out.shape[0] == max(0, min(at, 15) + c - 15) and fill == min(15, at + c)
            got.append(out)
            at += c
        assert np.array_equal(np.concatenate(got), a[:25]), cuts
    # counts and a fill above 15, the image of the restatement
    out, nout, new, keep = dab_time_deinterleave_numpy(b[16:], b[1:16], 99, n_frames=9)
    want = ref.deinterleave_image([b[16:].tolist()], [9], [b[1:16].tolist()], [99], n, 24, None, 0)
    assert nout == want[1][0] == 9 and keep == want[3][0] == 15 and np.array_equal(out, a[1:10])
    assert out.reshape(-1).tolist() == want[0][:9 * n] and new.reshape(-1).tolist() == want[2][0]


def test_puncture_and_depuncture():
    rng = np.random.default_rng(3)
    for p in (eep_profile("4-A", 1), eep_profile("2-A", 1), FIC_PROFILE):
        coded = rng.integers(1, 100, size=(2, p.steps, 4)).astype(np.int16)
        sent = dab_puncture_numpy(coded, p)
        mask = ref.mask_walk(p.segments)
        assert sent.shape == (2, p.n_received) and sent[1].tolist() == ref.puncture(coded[1].reshape(-1).tolist(), mask)
        back = dab_depuncture_numpy(sent, p)
        assert back.shape == coded.shape and back[1].reshape(-1).tolist() == ref.depuncture(sent[1].tolist(), mask)
        assert np.array_equal(back.reshape(2, -1), np.where(p.mask(), coded.reshape(2, -1), 0))
    with pytest.raises(ValueError):
        dab_depuncture_numpy(np.zeros((1, 5), dtype=np.int16), FIC_PROFILE)


def test_a_fic_block_through_encoder_puncturing_and_the_oracle(oracle):
    from oracle import pyoracle
    code = COMMON_CODES[4]
    assert (code.name, code.K, code.R) == ("DAB Radio", 7, 4)
    pc = get_decoding_config("SOFT16", 4)
    rng = np.random.default_rng(12)
    data = rng.integers(0, 256, size=(4, FIC_PROFILE.info_bits // 8), dtype=np.uint8)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, dab_energy_dispersal_numpy(data))
    assert coded.shape == (4, FIC_PROFILE.steps, 4)
    sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, None, 4, rng, pc.soft_dtype)
    assert pc.soft_decision_high + pc.soft_decision_low == 0       # 0 is the erasure
    received = dab_puncture_numpy(sym, FIC_PROFILE)
    assert received.shape == (4, 2304)
    back = dab_depuncture_numpy(received, FIC_PROFILE)
    got, _, _ = oracle.decode_frames(code.K, code.R, code.G, pyoracle.stock_config(pyoracle.SOFT16, 4), back, FIC_PROFILE.info_bits)
    assert np.array_equal(dab_energy_dispersal_numpy(got), data)


def test_the_kernel_source_on_the_host_under_the_sanitizers(tmp_path):
    """tests/cpp/dab_host_check.cpp: the kernels' device functions compiled by g++ with the HIP built-ins stubbed, as a program of its own
    -- with the address and undefined-behaviour sanitizers where g++ links them --, run as a child process: random shapes of both kernels
    whose buffers end their heap blocks, count, fill and map memory of every size, against a literal restatement.  In front of the shapes the
    program walks both argument rules: an accepted call, every INVALID_ARG case of tests/test_gpu_dab.py, the zero-work cases.  Only
    where the linker reports that it cannot find a sanitizer's runtime is the program built without them, and the test prints which build ran"""
    exe = str(tmp_path / "dab_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "dab_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("dab_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "300", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 300 shapes"), q.stdout
