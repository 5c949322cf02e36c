"""CPU side of the re-encoded channel symbol error count: the counting rule's numpy mirror (synth.channel_errors_numpy) on
hand-built cases, the Python encoders the GPU tests take their expected values from against the oracle's encoder (and both of the
reference's, where it is built), and the new entry points of the library (resolved, NULL handle rejected: no device needed)."""
import ctypes as C

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, _lib, get_decoding_config, synth


def _frames(code, decode_type, F, n_bytes, seed):
    pc = get_decoding_config(decode_type, code.R)
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(F, n_bytes), dtype=np.uint8)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, data)
    sym = np.where(coded != 0, pc.soft_decision_high, pc.soft_decision_low).astype(pc.soft_dtype)
    return pc, coded, sym


@pytest.mark.parametrize("decode_type", ["HARD8", "SOFT16"])
def test_counting_rule_on_hand_built_cases(decode_type):
    code = COMMON_CODES[2]
    pc, coded, sym = _frames(code, decode_type, 3, 5, 1)
    high, low = pc.soft_decision_high, pc.soft_decision_low
    n = sym[0].size
    assert n == (40 + code.K - 1) * code.R
    err, cmp = synth.channel_errors_numpy(code, high, low, sym, coded)
    assert err.tolist() == [0, 0, 0] and cmp.tolist() == [n, n, n]          # all symbols correct: (0, steps*R)
    # n flipped symbols give n, per frame
    flips = {0: [0, 1, n - 1], 1: [], 2: [17]}
    bad = sym.copy().reshape(3, -1)
    for f, where in flips.items():
        for k in where:
            bad[f, k] = high if bad[f, k] == low else low
    err, cmp = synth.channel_errors_numpy(code, high, low, bad.reshape(sym.shape), coded)
    assert err.tolist() == [3, 0, 1] and cmp.tolist() == [n, n, n]
    # a symbol at the midpoint is in neither number, whether it replaced a correct or a flipped symbol
    mid = (high + low) // 2
    assert 2 * mid == high + low
    bad[0, 1] = mid
    bad[0, 5] = mid
    bad[2, 40] = mid
    err, cmp = synth.channel_errors_numpy(code, high, low, bad.reshape(sym.shape), coded)
    assert err.tolist() == [2, 0, 1] and cmp.tolist() == [n - 2, n, n - 1]
    # a weak symbol still counts by its sign
    if decode_type == "SOFT16":
        weak = sym.copy().reshape(3, -1)
        weak[1, 3] = 1 if coded.reshape(3, -1)[1, 3] else -1
        weak[1, 4] = -1 if coded.reshape(3, -1)[1, 4] else 1
        err, cmp = synth.channel_errors_numpy(code, high, low, weak.reshape(sym.shape), coded)
        assert err.tolist() == [0, 1, 0] and cmp.tolist() == [n, n, n]


def test_counting_rule_with_an_off_centre_midpoint():
    """high + low odd: no symbol sits at the midpoint, the hard decision is 2 r > high + low"""
    code = COMMON_CODES[0]
    coded = np.array([[[1, 0], [0, 1]]], dtype=np.uint8)
    sym = np.array([[[1, 0], [1, 0]]], dtype=np.int8)              # high = 1, low = 0: 2 r > 1
    err, cmp = synth.channel_errors_numpy(code, 1, 0, sym, coded)
    assert err.tolist() == [2] and cmp.tolist() == [4]


@pytest.mark.parametrize("code_id", range(len(COMMON_CODES)))
def test_python_encoders_agree_with_the_oracle_and_the_reference(oracle, code_id, request):
    code = COMMON_CODES[code_id]
    rng = np.random.default_rng(100 + code_id)
    data = rng.integers(0, 256, size=(4, 9), dtype=np.uint8)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, data)
    for f in range(4):
        assert np.array_equal(coded[f].reshape(-1), oracle.encode(code.K, code.R, code.G, data[f])), (code.name, f)
    # tail-biting: the zero-start encoder, started K-1 bits early on the frame's own last bits, gives the same symbols
    bits = np.unpackbits(data, axis=1)[:, :67]
    tb = synth.encode_tail_biting_numpy(code.K, code.R, code.G, bits)
    for f in range(4):
        pre = np.concatenate([bits[f, 67 - (code.K - 1):], bits[f]])
        pre = np.concatenate([pre, np.zeros((-pre.size) % 8, dtype=np.uint8)])                        # whole bytes for the oracle
        full = oracle.encode(code.K, code.R, code.G, np.packbits(pre)).reshape(-1, code.R)
        assert np.array_equal(tb[f], full[code.K - 1:code.K - 1 + 67]), (code.name, f)
    from oracle import pyoracle
    if pyoracle.RefLib.available():
        reflib = request.getfixturevalue("reflib")
        assert reflib.stock_code(code_id)[1:] == (code.K, code.R, list(code.G))
        for which in (0, 1):
            for f in range(4):
                assert np.array_equal(coded[f].reshape(-1), reflib.encode(code_id, data[f], which=which)), (code.name, which, f)


def test_new_entry_points_resolve_and_reject_a_null_handle():
    lib = _lib.load()
    assert "vit_hip_encode_batch" in _lib.EXPORTS and "vit_hip_channel_errors_batch" in _lib.EXPORTS
    assert (_lib.ENCODE_TAIL, _lib.ENCODE_TAIL_BITING) == (1, 2)
    buf = np.zeros(64, dtype=np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.vit_hip_encode_batch(None, p, 0, 1, 8, _lib.ENCODE_TAIL, None, p, 0, None, None) == _lib.ERR_INVALID_ARG
    assert b"NULL handle" in lib.vit_hip_last_error()
    assert lib.vit_hip_channel_errors_batch(None, p, 0, p, 0, 1, 8, _lib.ENCODE_TAIL, None, p, p, None) == _lib.ERR_INVALID_ARG
    assert b"NULL handle" in lib.vit_hip_last_error()
    assert not buf.any()
