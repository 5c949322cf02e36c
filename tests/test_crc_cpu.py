"""The frame check on the host: the stock CRC codes against their published check values, crc_numpy against the polynomial long division
of tests/crc_reference.py, the transmit side, the error-detection guarantees of a CRC (every single-bit error; every burst no longer
than the width), CRCCode's argument rule, the ABI's answer to a NULL handle, and the kernel's own source run on the host under the
address and undefined-behaviour sanitizers (tests/cpp/crc_host_check.cpp).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import crc_reference as ref
from viterbidecodercpp_amd import (CCSDS_CRC16, DAB_CRC16, LTE_CRC8, LTE_CRC16, LTE_CRC24A, LTE_CRC24B, MPEG2_CRC32, STOCK_CRC_CODES, CRCCode,
                                   _lib, crc_append_numpy, crc_field_numpy, crc_numpy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = np.frombuffer(b"123456789", dtype=np.uint8)


@pytest.mark.parametrize("code,params,check", [
    (CCSDS_CRC16, (16, 0x1021, 0xFFFF, 0), 0x29B1),
    (LTE_CRC16, (16, 0x1021, 0, 0), 0x31C3),
    (DAB_CRC16, (16, 0x1021, 0xFFFF, 0xFFFF), 0xD64E),
    (LTE_CRC24A, (24, 0x864CFB, 0, 0), 0xCDE703),
    (LTE_CRC24B, (24, 0x800063, 0, 0), 0x23EF52),
    (LTE_CRC8, (8, 0x9B, 0, 0), 0xEA),
    (MPEG2_CRC32, (32, 0x04C11DB7, 0xFFFFFFFF, 0), 0x0376E6E7),
], ids=sorted(STOCK_CRC_CODES, key=list(STOCK_CRC_CODES).index))
def test_stock_codes_and_their_check_values(code, params, check):
    assert (code.width, code.poly, code.init, code.xorout) == params and code in STOCK_CRC_CODES.values()
    assert int(crc_numpy(code, CHECK, 72)) == check
    assert ref.crc_reference(code, CHECK, 72) == check
    assert len(STOCK_CRC_CODES) == 7


@pytest.mark.parametrize("width", ref.WIDTHS_CPU)
def test_crc_numpy_equals_the_long_division(width):
    rng = np.random.default_rng(width)
    for trial in range(12):
        code = ref.random_code(width, rng)
        n_bits = int(rng.choice([0, 1, 7, 8, 9, width - 1, width, 31, 32, 33, 64, 65, 240, 1000]))
        first_bit = int(rng.choice(ref.FIRST_BITS))
        frames = rng.integers(0, 256, size=(2, 3, (first_bit + n_bits + width + 7) // 8 + 2), dtype=np.uint8)
        got = crc_numpy(code, frames, n_bits, first_bit)
        field = crc_field_numpy(code, frames, n_bits, first_bit)
        assert got.shape == (2, 3) and got.dtype == np.int64
        for r in range(2):
            for f in range(3):
                assert int(got[r, f]) == ref.crc_reference(code, frames[r, f], n_bits, first_bit), (code, n_bits, first_bit)
                assert int(field[r, f]) == ref.field_reference(code, frames[r, f], n_bits, first_bit)
    assert int(crc_numpy(code, frames[0, 0], 0, 5)) == code.init ^ code.xorout


@pytest.mark.parametrize("width", ref.WIDTHS_CPU)
def test_append_gives_syndrome_zero_or_the_mask(width):
    rng = np.random.default_rng(100 + width)
    code = ref.random_code(width, rng)
    for n_bits, first_bit in ((27, 0), (40, 3), (0, 7), (64, 8), (129, 13)):
        data = rng.integers(0, 256, size=(5, (first_bit + n_bits + 7) // 8), dtype=np.uint8)
        sent = crc_append_numpy(code, data, n_bits, first_bit)
        assert sent.shape == (5, max((first_bit + n_bits + width + 7) // 8, data.shape[1]))
        end = first_bit + n_bits
        assert np.array_equal(np.unpackbits(sent, axis=1)[:, :end], np.unpackbits(data, axis=1)[:, :end])      # the bits in front stay
        assert not (crc_numpy(code, sent, n_bits, first_bit) ^ crc_field_numpy(code, sent, n_bits, first_bit)).any()
        mask = rng.integers(0, 1 << width, size=5)
        masked = crc_append_numpy(code, data, n_bits, first_bit, mask=mask)
        assert np.array_equal(crc_numpy(code, masked, n_bits, first_bit) ^ crc_field_numpy(code, masked, n_bits, first_bit), mask)
    with pytest.raises(ValueError):
        crc_append_numpy(code, data, n_bits, first_bit, mask=1 << width)


def _codewords_with(code, pattern_rows):
    """syndromes of one 64-data-bit codeword XORed with each row of bit patterns [k][64 + width]"""
    rng = np.random.default_rng(code.width)
    sent = crc_append_numpy(code, rng.integers(0, 256, size=8, dtype=np.uint8), 64)
    total = 64 + code.width
    bits = np.unpackbits(sent)[None, :total] ^ pattern_rows
    got = np.packbits(bits, axis=1)
    return crc_numpy(code, got, 64) ^ crc_field_numpy(code, got, 64)


@pytest.mark.parametrize("name", sorted(STOCK_CRC_CODES))
def test_every_single_bit_error_and_every_short_burst_is_detected(name):
    code = STOCK_CRC_CODES[name]
    total = 64 + code.width
    assert (_codewords_with(code, np.eye(total, dtype=np.uint8)) != 0).all()
    # a burst of length b <= width: first and last bit set, anything between, at every place
    patterns = []
    rng = np.random.default_rng(7)
    for b in range(2, code.width + 1):
        inner = [0, (1 << (b - 2)) - 1] + [int(x) for x in rng.integers(0, 1 << (b - 2), size=4)] if b > 2 else [0]
        for mid in set(inner):
            shape = [1] + [(mid >> k) & 1 for k in range(b - 2)] + [1]
            for at in range(total - b + 1):
                row = np.zeros(total, dtype=np.uint8)
                row[at:at + b] = shape
                patterns.append(row)
    assert (_codewords_with(code, np.array(patterns)) != 0).all()


def test_crccode_rejections():
    CRCCode(1, 1), CRCCode(32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), CRCCode(np.int64(8), np.uint32(7))
    for bad in ((0, 0), (33, 1), (8, 0x100), (8, 1, 0x100), (8, 1, 0, 0x100), (8, -1), (8, 1, -1), (8.0, 1), (8, "7"), (True, 1), (16, 0x1021, None)):
        with pytest.raises(ValueError):
            CRCCode(*bad)
    frames = np.zeros((2, 4), dtype=np.uint8)
    for bad in (dict(n_bits=33), dict(n_bits=17, first_bit=16), dict(n_bits=-1), dict(n_bits=8, first_bit=-1)):
        with pytest.raises(ValueError):
            crc_numpy(LTE_CRC16, frames, **bad)
    with pytest.raises(ValueError):
        crc_numpy(LTE_CRC16, frames.astype(np.int32), 8)
    with pytest.raises(ValueError):
        crc_field_numpy(LTE_CRC16, frames, 17)                     # the field would end behind the frame


def test_null_handle_through_the_abi():
    lib = _lib.load()
    assert "vit_hip_crc_batch" in _lib.EXPORTS
    params = _lib.VitHipCrcParams(16, 0x1021, 0xFFFF, 0)
    out = (C.c_uint32 * 4)(*([ref.POISON32] * 4))
    frames = (C.c_uint8 * 16)()
    rc = lib.vit_hip_crc_batch(None, C.byref(params), C.cast(frames, C.c_void_p), 0, 1, 4, None, 0, 16, C.cast(out, C.c_void_p), None, None)
    assert rc == _lib.ERR_INVALID_ARG and b"NULL" in lib.vit_hip_last_error()
    assert list(out) == [ref.POISON32] * 4


def test_kernel_source_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/crc_host_check.cpp: the kernel's device functions compiled by g++ with the HIP built-ins stubbed, one thread per block, as
    a program of its own -- with the address and undefined-behaviour sanitizers where g++ links them: frames and outputs in heap blocks
    that end with their last byte, every output against a bit-by-bit restatement.  In front of the shapes the
    program walks the argument rule: an accepted call, every INVALID_ARG case of tests/test_gpu_crc.py, the zero-work cases.  Only
    where the linker reports that it cannot find a sanitizer's runtime is the program built without them, and the test prints which build ran"""
    exe = str(tmp_path / "crc_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "crc_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("crc_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "600", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 600 shapes") and q.stdout.strip().endswith("0x7f"), q.stdout       # every group size 1 .. 64 was met
