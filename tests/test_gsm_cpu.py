"""viterbidecodercpp_amd/gsm.py against the literal check values of include/vit_hip.h and the independent restatement of
tests/gsm_reference.py: the code's impulse response, the interleaver maps, the de-interleaver with its history across every cut of a
sequence, the Fire code against the correction by definition, the TCH/FS frame, the three CRC constants, both receive chains over the CPU
oracle decoder at the recorded seed of sign flips; the argument errors the ABI reports without a device; and the kernels' own source with
their argument rules run on the host as a program of its own under the address and undefined-behaviour sanitizers
(tests/cpp/gsm_host_check.cpp).  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from viterbidecodercpp_amd import (COMMON_CODES, GSM_BLOCK, GSM_DIAGONAL, GSM_POLYNOMIALS, GSM_RACH_CRC6, GSM_SCH_CRC10, GSM_TCHFS_CRC3, _lib,
                                   crc_append_numpy, crc_field_numpy, crc_numpy, gsm_deinterleave_numpy, gsm_fire_encode_numpy, gsm_fire_numpy,
                                   gsm_interleave_map, gsm_tchfs_bursts_numpy, gsm_tchfs_class1_numpy, gsm_tchfs_numpy, gsm_xcch_bursts_numpy)
from viterbidecodercpp_amd.synth import encode_bits_numpy
from tests import gsm_cases as cases
from tests import gsm_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_impulse_response_of_the_code():
    assert GSM_POLYNOMIALS == (25, 27) == (0b11001, 0b11011) and COMMON_CODES[1].G == (23, 25)            # the stock set is as it was
    want = [[1, 1], [0, 1], [0, 0], [1, 1], [1, 1]]
    assert encode_bits_numpy(5, 2, GSM_POLYNOMIALS, np.array([[0x80]], dtype=np.uint8))[0, :5].tolist() == want
    pyoracle.ensure_built()
    assert pyoracle.Oracle().encode(5, 2, GSM_POLYNOMIALS, np.array([0x80], dtype=np.uint8)).reshape(-1, 2)[:5].tolist() == want
    # the oracle's decoder on the impulse's symbols returns the impulse
    sym = np.where(encode_bits_numpy(5, 2, GSM_POLYNOMIALS, np.array([[0x80]], dtype=np.uint8)) != 0, 127, -127).astype(np.int16)
    assert cases.decode(sym, 8).tolist() == [[0x80]]


def test_the_literal_checks_of_the_map():
    k = np.arange(456)
    j = 2 * ((49 * k) % 57) + (k % 8) // 4
    assert j[:8].tolist() == [0, 98, 82, 66, 51, 35, 19, 3]
    burst, element = gsm_interleave_map(GSM_BLOCK)
    assert burst.dtype == element.dtype == np.int32 and element.tolist() == np.where(j < 57, j, j + 2).tolist()
    assert sorted((burst * 114 + j).tolist()) == list(range(4 * 114))                                      # a bijection onto 4 x 114
    assert not set(element.tolist()) & {57, 58}
    burst8, element8 = gsm_interleave_map("diagonal")
    assert element8.tolist() == element.tolist() and burst8.tolist() == (k % 8).tolist()
    for b in range(8):                                                                                     # 57 a burst, even j first
        mine = j[burst8 == b]
        assert mine.size == 57 and len(set(mine.tolist())) == 57 and (mine % 2 == (b >= 4)).all()
    with pytest.raises(ValueError):
        gsm_interleave_map(2)
    # the forward scatter of the restatement lands every label where the map reads it
    for diagonal, (bs, el) in ((False, (burst, element)), (True, (burst8, element8))):
        bursts = ref.scatter([[(n, q) for q in range(456)] for n in range(3)], diagonal)
        assert all(bursts[4 * n + bs[q]][el[q]] == (n, q) for n in range(3) for q in range(456))


@pytest.mark.parametrize("dtype", [np.int16, np.int8])
def test_interleave_then_deinterleave_is_the_identity(dtype):
    rng = np.random.default_rng(5)
    info = np.iinfo(dtype)
    blocks = rng.integers(info.min, info.max + 1, size=(2, 5, 456)).astype(dtype)
    blocks[0, 0, :8] = info.min
    for mode in (GSM_BLOCK, GSM_DIAGONAL):
        diagonal = mode == GSM_DIAGONAL
        sent = np.array([[[0 if v is None else v for v in b] for b in ref.scatter(row.tolist(), diagonal)] for row in blocks], dtype=dtype)
        flags = rng.integers(-9, 10, size=sent.shape[:2] + (2,)).astype(dtype)
        sent[:, :, 57:59] = flags
        full, class1, class2, steal, n_out, hist, fill = gsm_deinterleave_numpy(sent, mode)
        m = sent.shape[1] // 4
        assert full.shape == (2, m, 228, 2) and class1.shape == (2, m, 189, 2) and class2.shape == (2, m, 78) and full.dtype == dtype
        got = full.reshape(2, m, 456)
        if diagonal:
            assert n_out.tolist() == [5, 5] and m == 6 and not got[:, 5].any() and not steal[:, 5].any()
            assert np.array_equal(hist, sent[:, -4:]) and fill.tolist() == [4, 4]
            want_steal = [[int(flags[r, 4 * n:4 * n + 4, 1].sum()) + int(flags[r, 4 * n + 4:4 * n + 8, 0].sum()) for n in range(5)] for r in range(2)]
        else:
            assert n_out.tolist() == [5, 5] and hist is None and fill is None
            want_steal = [[int(flags[r, 4 * n:4 * n + 4].sum()) for n in range(5)] for r in range(2)]
        assert np.array_equal(got[:, :5], blocks) and steal[:, :5].tolist() == want_steal
        assert np.array_equal(class1.reshape(2, m, 378), got[:, :, :378]) and np.array_equal(class2, got[:, :, 378:])
        negated = gsm_deinterleave_numpy(sent, mode, negate=True)
        assert np.array_equal(negated[0].reshape(2, m, 456)[:, :5], np.minimum(-blocks.astype(np.int32), info.max).astype(dtype))
        assert negated[3][:, :5].tolist() == (-np.array(want_steal)).tolist()
    for bad in (lambda: gsm_deinterleave_numpy(np.zeros((1, 5, 116), dtype=np.int16), GSM_BLOCK), lambda: gsm_deinterleave_numpy(np.zeros((1, 4, 115), dtype=np.int16), 0),
                lambda: gsm_deinterleave_numpy(np.zeros((1, 4, 116), dtype=np.int32), 0),
                lambda: gsm_deinterleave_numpy(np.zeros((1, 4, 116), dtype=np.int16), GSM_BLOCK, hist=np.zeros((1, 4, 116)), fill=[4]),
                lambda: gsm_deinterleave_numpy(np.zeros((1, 4, 116), dtype=np.int16), GSM_DIAGONAL, hist=np.zeros((1, 4, 116)))):
        with pytest.raises(ValueError):
            bad()


def test_the_history_across_every_cut_of_a_six_block_sequence():
    """6 blocks are 28 bursts = 7 groups of four: every way of cutting the 7 groups into consecutive calls, a start without history
    included, gives the 6 blocks in order, the first call one block less than its groups"""
    rng = np.random.default_rng(6)
    blocks = rng.integers(-127, 128, size=(6, 456)).astype(np.int16)
    sent = np.array([[0 if v is None else v for v in b] for b in ref.scatter(blocks.tolist(), True)], dtype=np.int16)
    assert sent.shape == (28, 116)
    cuts = 0
    for marks in itertools.product((False, True), repeat=6):
        edges = [0] + [i + 1 for i, cut in enumerate(marks) if cut] + [7]
        hist = fill = None
        got = []
        for a, b in zip(edges, edges[1:]):
            full, _, _, _, n_out, hist, fill = gsm_deinterleave_numpy(sent[None, 4 * a:4 * b], GSM_DIAGONAL, hist=hist, fill=fill)
            assert n_out[0] == b - a - (a == 0) and not full[0, n_out[0]:].any()
            got.append(full[0, :n_out[0]].reshape(-1, 456))
        assert np.array_equal(np.concatenate(got), blocks), marks
        cuts += 1
    assert cuts == 64
    # fill other than 4 means no history, whatever hist holds
    full, _, _, _, n_out, _, _ = gsm_deinterleave_numpy(sent[None, :8], GSM_DIAGONAL, hist=sent[None, 8:12], fill=[0])
    assert n_out[0] == 1 and np.array_equal(full[0, 0].reshape(-1), blocks[0])


def test_the_check_values_of_the_fire_code():
    assert ref.G == 0x10004820009 == sum(1 << p for p in (40, 26, 23, 17, 3, 0))
    d23 = (1 << 23) | 1                                                                                     # (D^23 + 1)(D^17 + D^3 + 1)
    product = 0
    for p in (17, 3, 0):
        product ^= d23 << p
    assert product == ref.G
    zero = gsm_fire_encode_numpy(np.zeros((1, 23), dtype=np.uint8))
    assert zero[0].tolist() == [0] * 23 + [0xFF] * 5                                                        # 184 zeros carry 40 ones
    status, data = gsm_fire_numpy(zero)
    assert status.tolist() == [[0, 0, 0, 0]] and not data.any()
    last, first_parity = zero.copy(), zero.copy()
    last[0, 27] ^= 0x01
    first_parity[0, 22] ^= 0x01
    assert gsm_fire_numpy(last, 0)[0].view(np.uint32).tolist() == [[0xFFFFFFFF, 0, 1, 0]]                   # u(223): syndrome 1
    assert gsm_fire_numpy(first_parity, 0)[0].view(np.uint32).tolist() == [[0xFFFFFFFF, 0, 0x04820009, 0]]  # u(183): 0x0004820009
    assert gsm_fire_numpy(last)[0].tolist() == [[1, 223, 1, 0]] and gsm_fire_numpy(first_parity)[0].tolist() == [[1, 183, 0x04820009, 0]]
    assert len(ref.patterns()) == 438271                                                                    # distinct and non-zero: asserted there
    top = zero.copy()
    top[0, 0] ^= 0x80                                                                                       # u(0): a syndrome above 2^32
    s = gsm_fire_numpy(top)[0].view(np.uint32)[0]
    assert (int(s[3]) << 32 | int(s[2])) == ref.syndrome(np.unpackbits(top[0]).tolist()) and s[3] != 0
    for bad in (lambda: gsm_fire_numpy(zero, 13), lambda: gsm_fire_numpy(zero[:, :27]), lambda: gsm_fire_encode_numpy(np.zeros((1, 22), dtype=np.uint8))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("max_burst", [0, 5, 12])
def test_the_fire_rule_against_the_correction_by_definition(max_burst):
    frames, sent = cases.fire_frames()
    status, data = gsm_fire_numpy(frames, max_burst)
    lsb = gsm_fire_numpy(frames, max_burst, lsb_first=True)[1]
    seen = set()
    for f in range(frames.shape[0]):
        want = ref.correct(np.unpackbits(frames[f]).tolist(), max_burst)
        got = status[f].view(np.uint32)
        assert (int(status[f, 0]), int(got[1]), int(got[3]) << 32 | int(got[2])) == want[:3], f
        assert np.unpackbits(data[f]).tolist() == want[3][:184], f
        assert np.unpackbits(lsb[f], bitorder="little").tolist() == want[3][:184], f
        seen.add(int(status[f, 0]))
        if 0 < status[f, 0] and f < 8 + 48 + 15:                                                            # the planted bursts come back
            assert np.array_equal(data[f], sent[f, :23]), f
    assert (status[:8, 0] == 0).all() and seen == ({0, -1} if max_burst == 0 else set(range(-1, max_burst + 1)))


def test_every_single_bit_error_is_corrected_where_it_is():
    sent = gsm_fire_encode_numpy(np.random.default_rng(9).integers(0, 256, size=(1, 23), dtype=np.uint8))
    bits = np.repeat(np.unpackbits(sent, axis=1), 224, axis=0)
    bits[np.arange(224), np.arange(224)] ^= 1
    status, data = gsm_fire_numpy(np.packbits(bits, axis=1), 1)
    assert status[:, 0].tolist() == [1] * 224 and status[:, 1].tolist() == list(range(224)) and (data == sent[0, :23]).all()
    assert [int(s[3]) << 32 | int(s[2]) for s in status.view(np.uint32)] == ref.single_bit_syndromes()


def test_the_tchfs_frame():
    rng = np.random.default_rng(11)
    decoded = rng.integers(0, 256, size=(9, 24), dtype=np.uint8)
    class2 = rng.integers(-127, 128, size=(9, 78)).astype(np.int16)
    class2[0, :5] = (0, 1, -1, 0, 127)                                                                     # two at the midpoint: bit 0, counted
    speech, status = gsm_tchfs_numpy(decoded, class2, 127, -127)
    assert speech.shape == (9, 33) and status.dtype == np.int32 and not (speech[:, 32] & 0x0F).any()
    for f in range(9):
        d, syndrome, erased = ref.tchfs(np.unpackbits(decoded[f]).tolist(), class2[f].tolist(), 127, -127)
        assert np.unpackbits(speech[f])[:260].tolist() == d and status[f].tolist() == [syndrome, erased], f
    assert np.unpackbits(speech[0])[182:187].tolist() == [0, 1, 0, 0, 1] and status[0, 1] >= 2
    # another midpoint: HARD8-like levels 1 / 0 -> 2 c > 1
    assert np.unpackbits(gsm_tchfs_numpy(decoded[:1], np.ones((1, 78), dtype=np.int8), 1, 0)[0][0])[182:260].all()
    # the transmit side makes the parity hold, and the reorder comes back
    sent = np.packbits(np.concatenate([rng.integers(0, 2, size=(4, 260), dtype=np.uint8), np.zeros((4, 4), dtype=np.uint8)], axis=1), axis=1)
    u = gsm_tchfs_class1_numpy(sent)
    back, st = gsm_tchfs_numpy(u, np.where(np.unpackbits(sent, axis=1)[:, 182:260] != 0, 127, -127), 127, -127)
    assert np.array_equal(back, sent) and not st.any()
    u[0, 0] ^= 0x80                                                                                         # d(0) is under the parity
    broken = gsm_tchfs_numpy(u, np.zeros((4, 78), dtype=np.int16), 127, -127)[1]
    assert broken[0, 0] != 0 and not broken[1:, 0].any() and broken[:, 1].tolist() == [78] * 4
    with pytest.raises(ValueError):
        gsm_tchfs_numpy(decoded[:, :23], class2, 127, -127)


@pytest.mark.parametrize("code,data_bits", [(GSM_SCH_CRC10, 25), (GSM_RACH_CRC6, 8), (GSM_TCHFS_CRC3, 50)], ids=["sch", "rach", "tchfs"])
def test_the_crc_constants_encode_and_check(code, data_bits):
    assert [tuple(vars(c).values()) for c in (GSM_SCH_CRC10, GSM_RACH_CRC6, GSM_TCHFS_CRC3)] == [(10, 0x175, 0, 0x3FF), (6, 0x2F, 0, 0x3F), (3, 0x3, 0, 0x7)]
    rng = np.random.default_rng(code.width)
    frames = rng.integers(0, 256, size=(16, 8), dtype=np.uint8)
    sent = crc_append_numpy(code, frames, data_bits)
    assert not (crc_numpy(code, sent, data_bits) ^ crc_field_numpy(code, sent, data_bits)).any()
    # the remainder of data and field together is all ones, as the standard words it: by long division with this code's polynomial
    poly = (1 << code.width) | code.poly
    for f in range(16):
        r = 0
        for b in np.unpackbits(sent[f])[:data_bits + code.width].tolist():
            r = (r << 1) | b
            if r >> code.width:
                r ^= poly
        assert r == (1 << code.width) - 1
    sent[3, 0] ^= 0x40
    assert (crc_numpy(code, sent, data_bits) ^ crc_field_numpy(code, sent, data_bits))[3] != 0
    if code is GSM_RACH_CRC6:                                                                               # the BSIC added to the parity comes out as the syndrome
        with_bsic = crc_append_numpy(code, frames, data_bits, mask=0x2A)
        assert (crc_numpy(code, with_bsic, data_bits) ^ crc_field_numpy(code, with_bsic, data_bits)).tolist() == [0x2A] * 16


def test_the_control_chain_over_the_oracle_decoder():
    bursts, l2, (got, status) = cases.control_set()
    assert bursts.shape == (1, 32, 116) and set(np.abs(bursts).reshape(-1).tolist()) == {127}
    clean = gsm_xcch_bursts_numpy(l2)
    assert (np.sign(bursts[0]) != np.sign(clean)).sum() == 8 * cases.FLIPS                                  # the decodes have work to do
    assert np.array_equal(got, l2) and (status[:, 0] == 0).all()
    lsb = cases.control_chain(bursts, lsb_first=True)[0]
    assert np.array_equal(np.unpackbits(lsb, axis=1, bitorder="little"), np.unpackbits(l2, axis=1))
    assert (gsm_deinterleave_numpy(bursts, GSM_BLOCK)[3] == 8 * 127).all()                                  # SACCH: every flag 1


def test_the_traffic_chain_over_the_oracle_decoder():
    bursts, speech, l2 = cases.traffic_set()
    assert bursts.shape == (36, 116)
    clean = gsm_tchfs_bursts_numpy(speech)
    assert (clean[:4, 1:57:2] == 0).all() and (clean[-4:, 0:57:2] == 0).all()                              # the halves no block fills
    for pushes in ([bursts[None]], [bursts[None, :12], bursts[None, 12:16], bursts[None, 16:]]):
        out = cases.traffic_chain(pushes)
        assert [int(o[5][0]) for o in out] == [p.shape[1] // 4 - (i == 0) for i, p in enumerate(pushes)]
        got = [np.concatenate([o[i][:o[5][0]] for o in out]) for i in range(5)]
        keep = np.arange(8) != cases.STOLEN
        assert np.array_equal(got[0][keep], speech[keep]) and not got[1][keep].any()                       # every speech frame, parity held
        assert np.array_equal(got[2][cases.STOLEN], l2) and got[3][cases.STOLEN, 0] == 0                    # the stolen block is the FACCH frame
        assert got[4].tolist() == [8 * 127 if n == cases.STOLEN else -8 * 127 for n in range(8)]
        assert (got[3][keep, 0] != 0).all()                                                                 # speech is no Fire codeword


def test_the_abi_rejects_without_a_device():
    lib = _lib.load()
    for name in ("vit_hip_gsm_deinterleave_batch", "vit_hip_gsm_fire_batch", "vit_hip_gsm_tchfs_batch"):
        assert name in _lib.EXPORTS
    buf = (C.c_uint8 * 64)(*([0x5A] * 64))
    at = C.cast(buf, C.c_void_p)
    assert lib.vit_hip_gsm_deinterleave_batch(None, at, 0, 0, 1, 4, 0, 0, None, None, None, None, None, at, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_gsm_fire_batch(None, at, 0, 1, 12, 0, at, at, 0, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error()
    assert lib.vit_hip_gsm_tchfs_batch(None, at, 0, at, 1, at, 0, None, None) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.vit_hip_last_error() and list(buf) == [0x5A] * 64
    kernels = _lib.list_kernels()
    for part in ("gsm_deinterleave_kernelIs", "gsm_deinterleave_kernelIa", "gsm_fire_kernel", "gsm_tchfs_kernelIs", "gsm_tchfs_kernelIa"):
        found = [r for name, r in kernels.items() if part in name]
        assert len(found) == 1 and found[0]["scratch_bytes"] == 0, part


def test_the_kernel_source_and_the_argument_rules_on_the_host(tmp_path):
    """tests/cpp/gsm_host_check.cpp: the kernels' functions and the argument rules compiled by g++ with the HIP built-ins stubbed, as a
    program of its own with the address and undefined-behaviour sanitizers, run as a child process.  Only where the linker reports that
    it cannot find a sanitizer's runtime is the program built without them; any other failure of the sanitizer build fails the test,
    and the test prints which build ran"""
    exe = str(tmp_path / "gsm_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "gsm_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("gsm_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "60", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 60 shapes"), q.stdout
