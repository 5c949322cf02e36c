"""viterbidecodercpp_amd/dvbt.py against the check values of include/vit_hip.h and the independent restatement of tests/dvbt_reference.py
at every mode, constellation, rate and parity; the transmit side undone by the receive rule; the spot rule; the steps per symbol; the
argument errors of the Python layer and the one the ABI reports without a device; and the kernel's own source with its argument rule run
on the host as a program of its own (tests/cpp/dvbt_host_check.cpp); and the case builders the GPU tests share (tests/dvbt_cases.py):
transmit() against the checksums of the values it had when it was part of tests/test_gpu_dvbt.py, its parity and decode type, the SNR
table against the standard's figures.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import (COMMON_CODES, DVBT_MODES, DVBT_RATES, _lib, dvbt_deinterleave_numpy, dvbt_interleave_numpy, dvbt_puncture_numpy,
                                   dvbt_steps_per_symbol, dvbt_symbol_permutation)
from tests import dvbt_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = {"2k": ([0, 1024, 16, 1025, 128, 1056, 2, 1280], 52702), "4k": ([0, 2048, 64, 2176, 1024, 2080, 256, 2050], 9494),
         "8k": ([0, 4096, 128, 4128, 2048, 4104, 1, 5120], 57713)}
ALL = [(m, v, r) for m in ("2k", "4k", "8k") for v in (2, 4, 6) for r in range(5)]


@pytest.mark.parametrize("mode", ["2k", "4k", "8k"])
def test_the_symbol_permutation(mode):
    h = dvbt_symbol_permutation(mode)
    m = DVBT_MODES[mode]
    assert h.shape == (m.n_max,) and (m.m_max, m.n_max, m.n_r) == {"2k": (2048, 1512, 11), "4k": (4096, 3024, 12), "8k": (8192, 6048, 13)}[mode]
    assert h[:8].tolist() == CHECK[mode][0]
    assert int((np.arange(h.size, dtype=np.int64) * h).sum() % 65521) == CHECK[mode][1]
    assert np.array_equal(np.sort(h), np.arange(m.n_max))
    assert h.tolist() == ref.h_table(mode)


def test_the_stock_code_is_y_then_x():
    assert COMMON_CODES[2].G == (109, 79) and (0o133, 0o171) != COMMON_CODES[2].G       # bit k taps the input of k steps ago: the octal read backwards
    assert tuple(int(format(g, "07b")[::-1], 2) for g in COMMON_CODES[2].G) == (0o133, 0o171)
    assert DVBT_RATES == ((1, 2), (2, 3), (3, 4), (5, 6), (7, 8))


def test_steps_per_symbol():
    assert dvbt_steps_per_symbol("2k", 2, 0) == 1512 and dvbt_steps_per_symbol("8k", 6, 4) == 31752
    for mode, v, rate in ALL:
        k, n = DVBT_RATES[rate]
        steps = dvbt_steps_per_symbol(mode, v, rate)
        assert steps * n == DVBT_MODES[mode].n_max * v * k and steps % k == 0 and steps == ref.steps_per_symbol(mode, v, rate)


@pytest.mark.parametrize("mode,v,rate", ALL, ids=["-".join(map(str, c)) for c in ALL])
def test_the_rule_against_the_reference_and_the_transmit_side(mode, v, rate):
    cell, steps = DVBT_MODES[mode].n_max * v, dvbt_steps_per_symbol(mode, v, rate)
    k = DVBT_RATES[rate][0]
    for parity in (0, 1):
        # labelled input: every soft value is its own index + 1, so any misplaced element shows
        x = np.arange(1, 2 * cell + 1, dtype=np.int32).reshape(1, 2, cell)
        got = dvbt_deinterleave_numpy(x, mode, v, rate, parity)
        assert got.shape == (1, 2 * steps, 2) and np.array_equal(got, ref.deinterleave(x, mode, v, rate, parity))
        # transmit side undone: kept positions come back, punctured ones are 0
        coded = np.arange(1, 4 * steps + 1, dtype=np.int32).reshape(2 * steps, 2)
        sent = dvbt_puncture_numpy(coded, rate)
        assert sent.size == 2 * cell
        back = dvbt_deinterleave_numpy(dvbt_interleave_numpy(sent, mode, v, parity), mode, v, rate, parity)
        kept = back != 0
        assert kept.sum() == sent.size and np.array_equal(back[kept], coded[kept])
        assert np.array_equal(kept.reshape(-1, 2 * k), np.broadcast_to(kept.reshape(-1, 2 * k)[0], (2 * steps // k, 2 * k)))
        assert np.array_equal(coded[kept], np.sort(sent))


def test_the_sent_order_of_every_rate():
    names = {0: "X1 Y1", 1: "X1 Y1 Y2", 2: "X1 Y1 Y2 X3", 3: "X1 Y1 Y2 X3 Y4 X5", 4: "X1 Y1 Y2 Y3 Y4 X5 Y6 X7"}
    for rate, text in names.items():
        k = DVBT_RATES[rate][0]
        coded = np.array([[f"Y{j + 1}", f"X{j + 1}"] for j in range(k)])
        assert " ".join(dvbt_puncture_numpy(coded, rate)) == text


def test_the_spot_rule():
    x = np.arange(1512 * 2, dtype=np.int32)[None]
    out = dvbt_deinterleave_numpy(x, "2k", 2, 0, 0)
    h = dvbt_symbol_permutation("2k")
    assert out[0, 1] == 0 and out[0, 0] == h[63] * 2 + 1            # out[0][1] = in[0][0][0], out[0][0] = in[0][H(63)][1]


def test_parity_per_row_and_one_row():
    rng = np.random.default_rng(3)
    x = rng.integers(-100, 100, size=(2, 3, 1512 * 4), dtype=np.int16)
    both = dvbt_deinterleave_numpy(x, "2k", 4, 2, [0, 1])
    assert np.array_equal(both[0], dvbt_deinterleave_numpy(x[0], "2k", 4, 2, 0)) and np.array_equal(both[1], dvbt_deinterleave_numpy(x[1], "2k", 4, 2, 1))
    assert np.array_equal(both, ref.deinterleave(x, "2k", 4, 2, [0, 1]))
    assert not np.array_equal(both[0], dvbt_deinterleave_numpy(x[0], "2k", 4, 2, 1))


def test_argument_errors():
    x = np.zeros((1, 1, 3024), dtype=np.int16)
    for bad in (lambda: dvbt_symbol_permutation("16k"), lambda: dvbt_deinterleave_numpy(x, "2k", 3, 0), lambda: dvbt_deinterleave_numpy(x, "2k", 2, 5),
                lambda: dvbt_deinterleave_numpy(x, "2k", 4, 0), lambda: dvbt_deinterleave_numpy(x[0, 0], "2k", 2, 0),
                lambda: dvbt_puncture_numpy(np.zeros((4, 2)), 2), lambda: dvbt_puncture_numpy(np.zeros((6, 3)), 2),
                lambda: dvbt_interleave_numpy(np.zeros(3023), "2k", 2), lambda: dvbt_steps_per_symbol("2k", 2, -1)):
        with pytest.raises(ValueError):
            bad()


# CRC-32 of (transport packets, soft bits) of transmit(mode, v, rate, 24, 11 + rate, SOFT16) noise-free and at (SNR_DB[rate], NOISE_SEED +
# rate), recorded when transmit() was part of tests/test_gpu_dvbt.py: the inputs of that file's chains
TRANSMIT_CRC = {("2k", 2, 0): ((26, 3024), 0xFD7D6650, 0xE57C7C4A, 0x62F1262E), ("2k", 2, 2): ((18, 3024), 0x4A565BD1, 0xA6AFB1C1, 0x851F051D),
                ("2k", 6, 4): ((5, 9072), 0xE3A3F9CF, 0xAFB00E58, 0xC017400E)}


def test_the_shared_transmit_side_is_the_recorded_one():
    import zlib

    from viterbidecodercpp_amd import get_decoding_config
    from tests import dvbt_cases as cases
    pc = get_decoding_config("SOFT16", 2)
    assert (cases.AMPLITUDE, cases.NOISE_SEED, cases.FORNEY_DELAY) == (48, 2024, 11)
    assert cases.SNR_DB == {0: 1.5, 1: 3.25, 2: 4.25, 3: 5.2, 4: 5.8}
    # EN 300 421 table 5: Eb/N0 for quasi-error-free reception by rate, plus 10 log10 of the rate, to the 0.05 dB the table is good for
    for rate, ebn0 in enumerate((4.5, 5.0, 5.5, 6.0, 6.4)):
        k, n = DVBT_RATES[rate]
        assert abs(cases.SNR_DB[rate] - (ebn0 + 10 * np.log10(k / n))) < 0.03, rate
    for (mode, v, rate), (shape, crc_ts, crc_clean, crc_noisy) in TRANSMIT_CRC.items():
        ts, clean = cases.transmit(mode, v, rate, 24, 11 + rate, pc)
        ts2, noisy = cases.transmit(mode, v, rate, 24, 11 + rate, pc, cases.SNR_DB[rate], cases.NOISE_SEED + rate)
        assert clean.shape == noisy.shape == shape and clean.dtype == noisy.dtype == np.int16 and ts.shape == (24, 188) and np.array_equal(ts, ts2)
        assert (zlib.crc32(ts.tobytes()), zlib.crc32(clean.tobytes()), zlib.crc32(noisy.tobytes())) == (crc_ts, crc_clean, crc_noisy), (mode, v, rate)


def test_the_shared_transmit_side_by_parity_and_decode_type():
    from viterbidecodercpp_amd import get_decoding_config
    from tests import dvbt_cases as cases
    pc = get_decoding_config("SOFT16", 2)
    ts, even = cases.transmit("2k", 4, 3, 4, 7, pc)
    ts1, odd = cases.transmit("2k", 4, 3, 4, 7, pc, parity=1)
    assert np.array_equal(ts, ts1) and even.shape == odd.shape and not np.array_equal(even, odd)
    steps = dvbt_deinterleave_numpy(even, "2k", 4, 3, 0)
    assert np.array_equal(steps, dvbt_deinterleave_numpy(odd, "2k", 4, 3, 1)) and not np.array_equal(steps, dvbt_deinterleave_numpy(odd, "2k", 4, 3, 0))
    assert np.array_equal(cases.transmit("2k", 4, 3, 4, 7, None, decode_type="SOFT16")[1], even)
    for decode_type, dtype, high in (("SOFT8", np.int8, None), ("HARD8", np.int8, 1)):
        levels = get_decoding_config(decode_type, 2)
        soft = cases.transmit("2k", 4, 3, 4, 7, None, decode_type=decode_type)[1]
        assert soft.dtype == dtype and (high is None or levels.soft_decision_high == high)
        assert np.array_equal(soft > 0, even > 0) and set(np.unique(soft)) == {levels.soft_decision_low, levels.soft_decision_high}
    # the host chain, noise-free, from either parity: 13 packets of 24 is a decode of 40 000 steps, so 12 packets of a short stream
    packets, status = cases.host_chain(cases.transmit("2k", 6, 4, 12, 8, pc, parity=1)[1], "2k", 6, 4, 12, parity=1)
    assert (status == 0).all() and np.array_equal(packets, cases.transmit("2k", 6, 4, 12, 8, pc)[0][:1])


def test_the_abi_reports_a_null_handle_without_a_device():
    lib = _lib.load()
    assert "vit_hip_dvbt_deinterleave_batch" in _lib.EXPORTS
    buf = (C.c_uint8 * 64)(*([0x5A] * 64))
    at = C.cast(buf, C.c_void_p)
    assert lib.vit_hip_dvbt_deinterleave_batch(None, at, 0, 1, 1, 0, 2, 0, 0, None, None, at, 0, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error() and list(buf) == [0x5A] * 64
    kernels = _lib.list_kernels()
    for part in ("dvbt_deinterleave_kernelIs", "dvbt_deinterleave_kernelIa"):
        found = [r for name, r in kernels.items() if part in name]
        assert len(found) == 1 and found[0]["scratch_bytes"] == 0, part


def test_the_kernel_source_and_the_argument_rule_on_the_host(tmp_path):
    """tests/cpp/dvbt_host_check.cpp: the kernel's functions and the argument rule compiled by g++ with the HIP built-ins stubbed, as a
    program of its own with the address and undefined-behaviour sanitizers, run as a child process.  Only where the linker reports that
    it cannot find a sanitizer's runtime is the program built without them; any other failure of the sanitizer build fails the test,
    and the test prints which build ran"""
    exe = str(tmp_path / "dvbt_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "dvbt_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("dvbt_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "90", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 90 shapes"), q.stdout
