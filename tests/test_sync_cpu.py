"""CPU side of node synchronisation: the hypothesis algebra of tests/sync_reference.py (the channel and its inverse hypothesis, the
build rule against depuncture's rule), the search on the reference alone -- it finds the true alignment with a margin, and the
inversion of a transparent code comes out as an exact tie resolved to the lower index --, the ranking, the hypothesis sets, and the
new entry points of the library (resolved, NULL handle rejected: no device needed)."""
import ctypes as C

import numpy as np
import pytest

from viterbidecodercpp_amd import COMMON_CODES, _lib, enumerate_hypotheses, get_decoding_config
from viterbidecodercpp_amd.sync import NEG_EVEN, NEG_ODD, SWAP
from tests import sync_reference as ref

ALL_FLAGS = range(8)


@pytest.mark.parametrize("decode_type", ["SOFT16", "SOFT8", "HARD8"])
@pytest.mark.parametrize("mask", [None, ref.MASK_3_4, (1, 0, 1, 1, 1, 1, 0, 1)])
def test_the_hypothesis_undoes_its_channel(decode_type, mask):
    """impair(offset, flags) then build_stream(offset, flags) restores the stream, for every flag set and offsets of both parities"""
    R = 2
    pc = get_decoding_config(decode_type, R)
    high, low = pc.soft_decision_high, pc.soft_decision_low
    rng = np.random.default_rng(7)
    T = 41
    stream = rng.integers(low, high + 1, size=(T, R)).astype(pc.soft_dtype)
    flat = stream.reshape(-1)
    keep = np.ones(flat.size, dtype=bool) if mask is None else np.resize(np.asarray(mask, dtype=bool), flat.size)
    want = np.where(keep, flat, 0).reshape(T, R)
    for offset in (0, 1, 2, 5):
        for flags in ALL_FLAGS:
            received = ref.impair(flat[keep], offset, flags, high, low, rng)
            got = ref.build_stream(received, offset, flags, T, R, high, low, mask)
            assert np.array_equal(got, want), (offset, flags)
            if flags:                                   # and another hypothesis does not
                assert not np.array_equal(ref.build_stream(received, offset, 0, T, R, high, low, mask), want)


def test_rotations_compose():
    """the four QPSK flag sets are the powers of one quarter turn: applying the turn's channel four times is the identity, twice is
    the inversion"""
    rng = np.random.default_rng(8)
    x = rng.integers(-127, 128, size=64).astype(np.int16)
    quarter = SWAP | NEG_EVEN
    y = x
    seen = []
    for _ in range(4):
        y = ref.impair(y, 0, quarter, 127, -127, rng, pad=0)
        seen.append(y.copy())
    assert np.array_equal(seen[3], x) and np.array_equal(seen[1], -x)
    # each power is undone by one hypothesis of the enumerated set
    for turned in seen:
        assert sum(np.array_equal(ref.build_stream(turned, 0, f, 32, 2, 127, -127).reshape(-1), x) for _, f in enumerate_hypotheses(1, "qpsk")) == 1


def test_negation_clamps_at_the_types_minimum():
    rec = np.array([-128, 127, -128, 5], dtype=np.int8)
    assert ref.build_stream(rec, 0, NEG_EVEN | NEG_ODD, 2, 2, 3, -3).reshape(-1).tolist() == [127, -127, 127, -5]
    rec16 = np.array([-32768, 1], dtype=np.int16)
    assert ref.build_stream(rec16, 0, NEG_EVEN, 1, 2, 127, -127).reshape(-1).tolist() == [32767, 1]


@pytest.mark.parametrize("R", [2, 3, 4])
def test_identity_hypothesis_is_depuncture(R):
    """offset 0, no flags, a mask: the numpy rule of BatchDecoder.depuncture applied period by period"""
    rng = np.random.default_rng(R)
    periods, steps = 7, 3
    mask = rng.integers(0, 2, size=steps * R).astype(bool)
    mask[0] = True
    kept = int(mask.sum())
    received = rng.integers(-127, 128, size=periods * kept).astype(np.int16)
    idx = np.where(mask, np.cumsum(mask) - 1, -1)                      # decoder.py: BatchDecoder.depuncture
    frames = received.reshape(periods, kept)
    want = np.where(idx >= 0, frames[:, np.maximum(idx, 0)], 0).reshape(periods * steps, R)
    assert np.array_equal(ref.build_stream(received, 0, 0, periods * steps, R, 127, -127, mask), want)
    src, k = ref.source_map(mask)
    assert k == kept and np.array_equal(src, idx)
    assert ref.needed_received([(0, 0)], periods * steps, R, mask) == received.size


def test_needed_received_is_the_largest_index_read():
    # without a map the bound is exact: a swap moves the last symbol of an even-length read one further only at an odd offset
    assert ref.needed_received([(0, 0)], 10, 2) == 20
    assert ref.needed_received([(0, SWAP)], 10, 2) == 20
    assert ref.needed_received([(1, 0)], 10, 2) == 21
    assert ref.needed_received([(1, SWAP)], 10, 2) == 22
    assert ref.needed_received([(0, 0), (2, NEG_ODD)], 10, 3) == 32
    # with a map a last partial period counts as a whole one: 3 whole periods of 4 kept and one more
    assert ref.needed_received([(0, 0)], 10, 2, ref.MASK_3_4) == 16
    assert ref.needed_received([(0, 0)], 9, 2, ref.MASK_3_4) == 12


def test_ranking_rule():
    assert ref.rank([5, 5, 4], [100, 100, 100]) == 2
    assert ref.rank([5, 5, 5], [100, 100, 100]) == 0                  # a tie: the lower index
    assert ref.rank([0, 3, 1], [0, 100, 50]) == 2                     # nothing compared loses to anything; 1/50 < 3/100
    assert ref.rank([0, 0], [0, 0]) == 0
    assert ref.rank([1, 2], [10, 20]) == 0                            # equal rates, exact in integers
    big = 2 ** 32 - 1
    assert ref.rank([big - 1, big - 2], [big, big - 1]) == 1          # (big-2)/(big-1) < (big-1)/big: needs the 64-bit product


def test_hypothesis_sets():
    assert enumerate_hypotheses(2) == [(0, 0), (1, 0)]
    assert enumerate_hypotheses(2, "bpsk") == [(0, 0), (0, 6), (1, 0), (1, 6)]
    assert enumerate_hypotheses(1, "qpsk") == [(0, 0), (0, SWAP | NEG_EVEN), (0, NEG_EVEN | NEG_ODD), (0, SWAP | NEG_ODD)]
    assert len(enumerate_hypotheses(4, "qpsk")) == 16
    with pytest.raises(ValueError):
        enumerate_hypotheses(2, "8psk")
    with pytest.raises(ValueError):
        enumerate_hypotheses(0)


def test_encoder_from_a_state_continues_the_zero_start_encoder():
    from viterbidecodercpp_amd import synth
    code = COMMON_CODES[ref.IS95]
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, size=6, dtype=np.uint8)
    bits = np.unpackbits(data)
    whole = synth.encode_bits_numpy(code.K, code.R, code.G, data)[0]
    cut = 16
    state = sum(int(bits[cut - 1 - j]) << j for j in range(code.K - 1))
    assert np.array_equal(ref.encode_from_state(code, bits[cut:], state), whole[cut:bits.size])
    assert ref.skip_bits(7) == 8 and ref.skip_bits(9) == 8 and ref.skip_bits(10) == 16 and ref.skip_bits(15) == 16


@pytest.mark.parametrize("name", ref.CPU_CASES)
def test_the_reference_finds_the_truth(oracle, name):
    """the winner is the true (offset, rotation) up to the inversion of a transparent code, with at most half the error rate of the
    best hypothesis that is not equivalent; the inversion ties exactly and the lower index wins; the winner's bits are the data"""
    c = ref.make_case(name)
    code, hyps, truth = c["code"], c["hypotheses"], c["truth"]
    errors, compared, best, decoded = ref.case_reference(oracle, name)
    assert ref.skip_bits(code.K) == {"is95": 8, "cassini": 16}.get(name, 8)
    assert ref.equivalent(code, hyps[best], truth), (hyps[best], truth)
    others = [i for i in range(len(hyps)) if not ref.equivalent(code, hyps[i], truth)]
    assert others and all(compared > 0)
    # errors_best / compared_best <= 1/2 * errors_i / compared_i
    assert all(2 * errors[best] * compared[i] <= errors[i] * compared[best] for i in others), list(zip(errors, compared))
    twins = [i for i in range(len(hyps)) if ref.equivalent(code, hyps[i], truth)]
    if ref.is_transparent(code) and len(twins) == 2:
        assert errors[twins[0]] == errors[twins[1]] and compared[twins[0]] == compared[twins[1]]
        assert best == min(twins)
        assert np.array_equal(decoded[twins[0]] ^ 1, decoded[twins[1]])
    else:
        assert twins == [c["true_index"]] == [best]
    tx = c["tx_bits"][c["head"]:c["T"] - c["tail"]]
    assert np.array_equal(decoded[c["true_index"]], tx)


def test_cases_cover_what_they_claim():
    assert ref.is_transparent(COMMON_CODES[ref.VOYAGER]) and ref.is_transparent(COMMON_CODES[ref.IS95])
    assert ref.make_case("voyager_3_4")["T"] * 2 % len(ref.MASK_3_4) != 0          # T R is not a multiple of the period
    assert ref.make_case("voyager")["T"] == 48 + 4 * 64 + 48
    long = ref.make_case("voyager_long")
    assert (long["T"] - long["head"] - long["tail"]) % long["W"] != 0              # a longer last window


def test_new_entry_points_resolve_and_reject_a_null_handle():
    lib = _lib.load()
    for name in ("vit_hip_sync_build", "vit_hip_sync_search_workspace_bytes", "vit_hip_sync_search"):
        assert name in _lib.EXPORTS and getattr(lib, name)
    assert (_lib.SYNC_SWAP_PAIRS, _lib.SYNC_NEGATE_EVEN, _lib.SYNC_NEGATE_ODD) == (1, 2, 4)
    assert C.sizeof(_lib.VitHipSyncHypothesis) == 8
    buf = np.zeros(64, dtype=np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    hyp = (_lib.VitHipSyncHypothesis * 1)((0, 0))
    assert lib.vit_hip_sync_build(None, p, 32, None, 0, 0, hyp, 1, 4, 4, p, None) == _lib.ERR_INVALID_ARG
    assert b"NULL handle" in lib.vit_hip_last_error()
    assert lib.vit_hip_sync_search(None, p, 32, None, 0, 0, hyp, 1, 4, 8, 6, 6, p, 64, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert b"NULL handle" in lib.vit_hip_last_error()
    assert lib.vit_hip_sync_search_workspace_bytes(None, 1, 352, 64, 48, 48) == 0
    assert not buf.any()
