"""viterbidecodercpp_amd/wifi.py against the independent restatement of tests/wifi_reference.py at all eight rates, the check values of
include/vit_hip.h, the order of the polynomials by an impulse through the package's encoder rule, the two statements of the FCS against
zlib, a round trip over the CPU oracle decoder, the argument errors the ABI reports without a device, and the kernels' own source run on
the host under the address and undefined-behaviour sanitizers (tests/cpp/wifi_host_check.cpp).  No GPU."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from viterbidecodercpp_amd import (WIFI_FCS, WIFI_POLYNOMIALS, WIFI_RATES, _lib, crc_field_numpy, crc_numpy, wifi_deinterleave_numpy,
                                   wifi_descramble_numpy, wifi_interleave_map, wifi_ppdu_numpy, wifi_scrambler_numpy, wifi_signal_field_numpy,
                                   wifi_signal_parse_numpy)
from viterbidecodercpp_amd.synth import encode_bits_numpy
from tests import wifi_cases as cases
from tests import wifi_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rate_table():
    assert len(WIFI_RATES) == 8
    for m, r in enumerate(WIFI_RATES):
        mbps, n_bpsc, mask, n_cbps, n_dbps, pattern = ref.RATES[m]
        assert (r.mbps, r.n_bpsc, r.n_cbps, r.n_dbps, list(r.signal_bits)) == (mbps, n_bpsc, n_cbps, n_dbps, pattern)
        assert r.n_cbps == 48 * r.n_bpsc and r.n_dbps * r.code_rate[1] == r.n_cbps * r.code_rate[0] and r.s == max(r.n_bpsc // 2, 1)
        assert sum(mask) * r.code_rate[0] * 2 == len(mask) * r.code_rate[1]


@pytest.mark.parametrize("rate", range(8))
def test_the_interleaver_map_equals_the_two_permutations(rate):
    got = wifi_interleave_map(rate)
    assert got.dtype == np.int32 and got.tolist() == ref.interleave_table(rate)
    assert sorted(got.tolist()) == list(range(WIFI_RATES[rate].n_cbps))


def test_the_check_values():
    assert wifi_interleave_map(0)[1] == 3 and wifi_interleave_map(4)[1] == 13
    assert np.packbits(wifi_scrambler_numpy(0b0000111, 16)).tolist() == [0x0E, 0xF2]
    assert ref.shift_register([1] * 7, 16) == np.unpackbits(np.array([0x0E, 0xF2], dtype=np.uint8)).tolist()     # the all-ones state
    seq = wifi_scrambler_numpy(0b1011101, 300)
    assert np.array_equal(seq[127:254], seq[:127]) and seq[:127].sum() == 64
    with pytest.raises(ValueError):
        wifi_interleave_map(8)


def test_the_polynomial_order_by_an_impulse():
    """an impulse through the package's encoder rule: output A is 1 at delays 0, 2, 3, 5, 6 and B at 0, 1, 2, 3, 6 (g0 = 133, g1 = 171)"""
    coded = encode_bits_numpy(7, 2, WIFI_POLYNOMIALS, np.array([[0x80]], dtype=np.uint8))[0]
    assert coded[:7, 0].tolist() == [1, 0, 1, 1, 0, 1, 1] and coded[:7, 1].tolist() == [1, 1, 1, 1, 0, 0, 1]
    assert not coded[7:].any()
    assert [int(format(g, "07b")[::-1], 2) for g in WIFI_POLYNOMIALS] == [0o133, 0o171]


@pytest.mark.parametrize("rate", range(8))
def test_the_deinterleave_rule_equals_the_walk(rate):
    rng = np.random.default_rng(rate)
    r, max_sym = WIFI_RATES[rate], 3
    soft = rng.integers(-128, 128, size=(6, max_sym * 288)).astype(np.int8)
    n_sym = [3, 2, 1, 0, 7, 3]
    n_steps = [10 ** 6, r.n_dbps + 5, r.n_dbps - 1, 9, 2 * r.n_dbps + 7, 3 * r.n_dbps - 2]
    for S in (3 * 216, 2 * r.n_dbps + 1, 5):
        got = wifi_deinterleave_numpy(soft, max_sym, S, rate=rate, n_sym=n_sym, n_steps=n_steps)
        assert got.dtype == np.int8 and got.shape == (6, S, 2)
        for f in range(6):
            assert got[f].reshape(-1).tolist() == ref.deinterleave(soft[f].tolist(), rate, max_sym, S, n_sym[f], n_steps[f]), (S, f)
    whole = wifi_deinterleave_numpy(soft, max_sym, 3 * r.n_dbps, rate=rate)
    assert whole[0].reshape(-1).tolist() == ref.deinterleave(soft[0].tolist(), rate, max_sym, 3 * r.n_dbps)
    kept = whole[0].reshape(-1)[np.tile(np.asarray(ref.RATES[rate][2]), 6 * r.n_dbps // len(ref.RATES[rate][2])) != 0]
    assert sorted(kept.tolist()) == sorted(soft[0, :3 * r.n_cbps].tolist())        # every soft bit of the three symbols, once


def test_mixed_and_invalid_rates_in_one_call():
    rng = np.random.default_rng(9)
    soft = rng.integers(-127, 128, size=(10, 2 * 288)).astype(np.int16)
    rates = [0, 1, 2, 3, 4, 5, 6, 7, 8, 2 ** 32 - 1]
    got = wifi_deinterleave_numpy(soft, 2, 432, rate=rates)
    for f, m in enumerate(rates):
        assert got[f].reshape(-1).tolist() == ref.deinterleave(soft[f].tolist(), m, 2, 432)
    assert not got[8:].any()


def test_the_signal_field_and_its_parser():
    for rate in range(8):
        for length in (1, 4, 100, 1500, 4095):
            bits = np.zeros(24, dtype=np.uint8)
            bits[:4] = ref.RATES[rate][5]
            bits[5:17] = [(length >> i) & 1 for i in range(12)]
            bits[17] = bits[:17].sum() % 2
            packed = np.packbits(bits)[None, :]
            want = ref.signal_parse(packed[0].tolist())
            assert wifi_signal_parse_numpy(packed).tolist() == [list(want)] and want[0] == rate and want[1] == length and want[4] == 1
            assert want[3] == 22 + 8 * length and want[2] == -(-want[3] // WIFI_RATES[rate].n_dbps)
            sent = wifi_signal_field_numpy(rate, length)
            assert sent.shape == (48,) and set(np.abs(sent).tolist()) == {127}
            sym = wifi_deinterleave_numpy(sent[None, :], 1, 24, rate=0)
            assert np.array_equal(sym[0] > 0, encode_bits_numpy(7, 2, WIFI_POLYNOMIALS, packed)[0, :24] != 0)
    rng = np.random.default_rng(3)
    fields = rng.integers(0, 256, size=(500, 3), dtype=np.uint8)
    fields[0] = (0xD0, 0x00, 0x00)                                 # 6 Mbit/s, length 0: not valid
    got = wifi_signal_parse_numpy(fields)
    assert got.dtype == np.uint32 and got.tolist() == [list(ref.signal_parse(f.tolist())) for f in fields]
    assert got[0].tolist() == [0, 0, 0, 0, 0] and 0 < got[:, 4].sum() < 500 and (got[:, 0] == 8).any()
    assert 1366 == ref.signal_parse(np.packbits(np.array([1, 1, 0, 1, 0] + [1] * 12 + [1], dtype=np.uint8)).tolist() + [0])[2]


def test_the_descramble_rule_equals_the_shift_register():
    rng = np.random.default_rng(4)
    for S, max_length in ((22, 4095), (30, 4095), (22 + 8 * 70 + 3, 4095), (22 + 8 * 70, 40), (1000, 4095)):
        nb = (S - 6 + 7) // 8
        data = rng.integers(0, 256, size=(9, nb + 2), dtype=np.uint8)
        data[1, 0] &= 1                                           # seven zero bits in front: seed 0
        lengths = [0, 3, 4, 5, 63, 64, 65, 4095, 2 ** 32 - 1]
        octets, status = wifi_descramble_numpy(data, S, lengths, max_length)
        assert status.dtype == np.uint32
        for f in range(9):
            want_psdu, want_status = ref.descramble(data[f].tolist(), S, lengths[f], max_length)
            assert octets[f].tobytes() == want_psdu and status[f].tolist() == list(want_status), (S, f)
        assert status[1, 1] == 0 and (status[2:, 1] > 0).all()
        assert (status[status[:, 0] < 4, 3] == 0xFFFFFFFF).all()


def test_the_two_statements_of_the_fcs_agree():
    """zlib.crc32 over the octets ^ their last four read little-endian == the 32-bit reversal of the non-reflected WIFI_FCS over the same
    bits in transmit order ^ the 32 bits behind them, MSB-first"""
    rng = np.random.default_rng(5)
    assert (WIFI_FCS.width, WIFI_FCS.poly, WIFI_FCS.init, WIFI_FCS.xorout) == (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF)
    for length in (4, 5, 7, 8, 9, 100):
        for good in (True, False):
            psdu = cases.with_fcs(rng.integers(0, 256, size=length - 4, dtype=np.uint8).tobytes()).copy()
            if not good:
                psdu[rng.integers(0, length)] ^= 1 << rng.integers(0, 8)
            frame = np.concatenate([np.zeros(2, dtype=np.uint8), np.packbits(np.unpackbits(psdu, bitorder="little"))])     # transmit order
            n = 8 * (length - 4)
            transmit = int(crc_numpy(WIFI_FCS, frame, n, 16)) ^ int(crc_field_numpy(WIFI_FCS, frame, n, 16))
            by_zlib = zlib.crc32(psdu[:-4].tobytes()) ^ int.from_bytes(psdu[-4:].tobytes(), "little")
            assert int(format(transmit, "032b")[::-1], 2) == by_zlib and (by_zlib == 0) == good


def _round_trip(specs, max_sym):
    signal_soft, data_soft, psdus = cases.make_ppdus(specs, max_sym, seed=len(specs))
    image, status, signal = cases.cpu_chain(signal_soft, data_soft, max_sym)
    for f, (rate, length, scr) in enumerate(specs):
        assert signal[f].tolist() == [rate, length, -(-(22 + 8 * length) // WIFI_RATES[rate].n_dbps), 22 + 8 * length, 1], (f, specs[f])
        assert status[f].tolist() == [length, scr, 0, 0 if length >= 4 else 0xFFFFFFFF], (f, specs[f])
        assert image[f, :length].tobytes() == psdus[f].tobytes() and (image[f, length:] == cases.FILL).all()


def test_round_trip_over_the_oracle_decoder_lengths():
    """lengths 1 (written, nothing to check), 4, 5, 100 and the largest that fits three OFDM symbols, at every rate"""
    specs = [(rate, length, 1 + (7 * rate + length) % 127) for rate in range(8) for length in (1, 4, 5, 100, cases.largest_length(rate, 3))]
    _round_trip(specs, 35)


def test_round_trip_every_seed():
    _round_trip([(5, 60, seed) for seed in range(1, 128)], 4)


def test_the_abi_rejects_without_a_device():
    lib = _lib.load()
    for name in ("vit_hip_wifi_deinterleave_batch", "vit_hip_wifi_signal_batch", "vit_hip_wifi_data_batch"):
        assert name in _lib.EXPORTS
    buf = (C.c_uint8 * 64)(*([0x5A] * 64))
    at = C.cast(buf, C.c_void_p)
    assert lib.vit_hip_wifi_deinterleave_batch(None, at, 0, 1, 1, 0, None, None, None, 0, 4, at, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_wifi_signal_batch(None, at, 0, 1, at, None) == _lib.ERR_INVALID_ARG and b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_wifi_data_batch(None, at, 0, 1, 64, at, 0, 4, at, 0, at, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert list(buf) == [0x5A] * 64
    kernels = _lib.list_kernels()
    for part in ("wifi_deinterleave_kernelIs", "wifi_deinterleave_kernelIa", "wifi_signal_kernel", "wifi_data_kernel"):
        found = [r for name, r in kernels.items() if part in name]
        assert len(found) == 1 and found[0]["scratch_bytes"] == 0, part


def test_the_kernel_source_on_the_host_under_the_sanitizers(tmp_path):
    """tests/cpp/wifi_host_check.cpp: the kernels' device functions compiled by g++ with the HIP built-ins stubbed, as a program of its own
    -- with the address and undefined-behaviour sanitizers where g++ links them --, run as a child process: random shapes with hostile
    rates, counts and lengths whose buffers end their heap blocks, every output byte against a literal restatement.  In front of the shapes the
    program walks the three argument rules: an accepted call, every INVALID_ARG case of tests/test_gpu_wifi.py, the zero-work cases.  Only
    where the linker reports that it cannot find a sanitizer's runtime is the program built without them, and the test prints which build ran"""
    exe = str(tmp_path / "wifi_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "wifi_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("wifi_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "300", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 300 shapes"), q.stdout
