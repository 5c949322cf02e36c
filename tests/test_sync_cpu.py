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


@pytest.mark.parametrize("name,errors,compared,winner", ref.RANK_SETS, ids=[r[0] for r in ref.RANK_SETS])
def test_hand_written_rankings(name, errors, compared, winner):
    """the sets tests/test_gpu_sync_kernels.py gives to sync_pick_kernel, with the winners spelled out in the list"""
    assert len(errors) == len(compared) and 1 <= len(errors) <= ref.MAX_HYPOTHESES
    assert all(0 <= e <= c < 2 ** 32 for e, c in zip(errors, compared))
    assert ref.rank(errors, compared) == winner


def test_hand_written_rankings_hold_their_premises():
    """equal rates are equal and their denominators are not; the wrap pairs need the whole 64-bit product"""
    sets = {name: (errors, compared, winner) for name, errors, compared, winner in ref.RANK_SETS}
    e, c, w = sets["equal rates, other denominators"]
    tied = [i for i in range(len(e)) if e[i] * c[w] == e[w] * c[i]]
    assert tied == [1, 3, 5] and len({c[i] for i in tied}) == 3
    low = 0xFFFFFFFF
    for ea, ca, eb, cb in (ref.WRAP_MORE_ERRORS, ref.WRAP_FEWER_COMPARED):
        assert max(ea, ca, eb, cb) < 2 ** 32 and abs(ea - eb) + abs(ca - cb) == 1
        assert ea * cb < eb * ca and (ea * cb) & low > (eb * ca) & low
    ea, ca, eb, cb = ref.WRAP_EQUAL_LOW
    assert ea * cb < eb * ca and (ea * cb) & low == (eb * ca) & low
    # in the list the better of each pair stands behind the worse: a ranking that sees a tie, or the other order, names index 0
    for name in ("one more error, low halves the other way", "one compared fewer, low halves the other way", "products 2^32 apart"):
        assert sets[name][2] == 1
    e, c, w = sets["64, the winner last"]
    assert len(e) == 64 and w == 63 and sum(ei * c[w] <= e[w] * ci for ei, ci in zip(e, c)) == 1      # unique


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
    assert ref.skip_bits(code.K) == {"is95": 8, "cassini": 16, "k11_lds2": 16}.get(name, 8)
    assert ref.equivalent(code, hyps[best], truth), (hyps[best], truth)
    others = [i for i in range(len(hyps)) if not ref.equivalent(code, hyps[i], truth)]
    assert others and all(compared > 0)
    # errors_best / compared_best <= 1/2 * errors_i / compared_i
    assert all(2 * errors[best] * compared[i] <= errors[i] * compared[best] for i in others), list(zip(errors, compared))
    twins = [i for i in range(len(hyps)) if ref.equivalent(code, hyps[i], truth)]
    if ref.is_transparent(code) and len(twins) == 2:
        assert errors[twins[0]] == errors[twins[1]] and compared[twins[0]] == compared[twins[1]]
        assert best == min(twins)
        if name == "voy34_hard8":
            # hard decisions behind a puncturing mask leave codewords that agree with every symbol that is compared: both twins
            # count no error at all, but the add-compare-select ties between such codewords go to the lower state, which an
            # inversion does not preserve -- the inverted twin decodes five bits of another codeword (bits 253 .. 262 of 295)
            assert errors[twins[0]] == 0 and np.count_nonzero((decoded[twins[0]] ^ 1) != decoded[twins[1]]) == 5
        else:
            assert np.array_equal(decoded[twins[0]] ^ 1, decoded[twins[1]])
    else:
        assert twins == [c["true_index"]] == [best]
    tx = c["tx_bits"][c["head"]:c["T"] - c["tail"]]
    assert np.array_equal(decoded[c["true_index"]], tx)


def test_cases_cover_what_they_claim(oracle):
    assert ref.is_transparent(COMMON_CODES[ref.VOYAGER]) and ref.is_transparent(COMMON_CODES[ref.IS95])
    # every width is searched, at R = 2, 3 and 4, with and without a mask
    assert {(ref.make_case(n)["decode_type"], ref.make_case(n)["code"].R) for n in ref.CPU_CASES} >= {
        ("SOFT16", 2), ("SOFT16", 3), ("SOFT8", 2), ("SOFT8", 3), ("HARD8", 2), ("HARD8", 4)}
    assert ref.make_case("voy34_hard8")["mask"] is not None and ref.make_case("voy34_hard8")["decode_type"] == "HARD8"
    # HARD8: the channel's noise lands on the midpoint, so the hypotheses compare different numbers of symbols and the ranking's
    # cross-multiplication has two denominators to work with
    compared = ref.case_reference(oracle, "voy_hard8")[1]
    assert len(set(compared.tolist())) > 1, compared
    # a state narrower than a byte; a state of 10 bits out of two skipped bytes, on a code outside the stock table
    k5, k11 = ref.make_case("k5")["code"], ref.make_case("k11_lds2")["code"]
    assert (k5.K, ref.skip_bits(k5.K)) == (5, 8) and (k11.K, ref.skip_bits(k11.K)) == (11, 16) and k11 not in COMMON_CODES
    assert [ref.make_case(n)["T"] for n in ("voy_soft8", "voy_hard8", "lte_soft8", "dab_hard8", "voy34_hard8")] == [352, 352, 357, 355, 359]
    assert ref.make_case("voyager_3_4")["T"] * 2 % len(ref.MASK_3_4) != 0          # T R is not a multiple of the period
    assert ref.make_case("voyager")["T"] == 48 + 4 * 64 + 48
    long = ref.make_case("voyager_long")
    assert (long["T"] - long["head"] - long["tail"]) % long["W"] != 0              # a longer last window


def test_random_rankings_hold_their_premise():
    """the seed of the random sets tests/test_gpu_sync_kernels.py ranks on the device: at least a third of the small-integer sets
    have two or more hypotheses tied for the best rate, both ends of n occur, and index 0 is not the usual winner"""
    sets = ref.random_rank_sets()
    assert len(sets) == 2000 and all(1 <= len(e) == len(c) <= ref.MAX_HYPOTHESES and (e <= c).all() for e, c in sets)
    small, wide = sets[0::2], sets[1::2]
    assert all(int(c.max()) <= 6 for _, c in small) and any(int(c.max()) >= 2 ** 31 for _, c in wide)
    ties = sum(1 for e, c in small if ref.tied_for_first(e, c) >= 2)
    assert 3 * ties >= len(small), f"only {ties} of {len(small)} small-integer sets tie for first place"
    assert any(len(e) == 1 for e, _ in sets) and any(len(e) == ref.MAX_HYPOTHESES for e, _ in sets)
    winners = [ref.rank([int(x) for x in e], [int(x) for x in c]) for e, c in sets]
    assert sum(1 for w in winners if w > 0) > len(sets) // 2


@pytest.mark.parametrize("name", ["voyager_64", "voyager_64_reversed", "voyager_1"])
def test_hypothesis_counts_on_the_reference(oracle, name):
    """64 hypotheses (offsets over four steps, all 8 flag sets), the same list reversed and the truth alone: the winner is the true
    alignment or the same one whole steps later, at half the rate of every other alignment; reversing the list moves the winner"""
    c = ref.make_case(name)
    hyps = c["hypotheses"]
    errors, compared, best, _ = ref.case_reference(oracle, name)
    assert len(hyps) == {"voyager_1": 1}.get(name, 64) and all(compared > 0)
    assert ref.aligned(c, hyps[best]), hyps[best]
    others = [i for i in range(len(hyps)) if not ref.aligned(c, hyps[i])]
    assert len(others) == len(hyps) - {"voyager_1": 1}.get(name, 8)
    assert all(2 * errors[best] * compared[i] <= errors[i] * compared[best] for i in others)
    if name == "voyager_64_reversed":
        forward = ref.case_reference(oracle, "voyager_64")
        assert errors.tolist() == forward[0].tolist()[::-1] and best != forward[2]
    if name == "voyager_1":
        assert best == 0


@pytest.mark.parametrize("name,residue", ref.SHAPE_CASES)
def test_extension_and_window_shapes_on_the_reference(oracle, name, residue):
    """the parameters of the extensions-and-windows test of tests/test_gpu_sync_search.py: they are what they claim, and the reference
    decodes and counts them by itself and still names the truth"""
    c = ref.make_case(name)
    K, R = c["code"].K, c["code"].R
    head, tail, W, T = c["head"], c["tail"], c["W"], c["T"]
    assert K == 7 and head != tail and {head, tail} <= {K - 1, K, 2 * K + 1, 8 * (K - 1)}
    assert W % head != 0 and W >= max(head, tail, 8)
    assert (T - head - tail) % W in (1, W - 1) and (T - head - tail) // W >= 2
    offset = (head + ref.skip_bits(K)) * R * np.dtype(c["pc"].soft_dtype).itemsize
    assert ref.residue_class(offset) == residue, offset
    errors, compared, best, decoded = ref.case_reference(oracle, name)
    assert all(d.size == T - head - tail for d in decoded) and all(compared > 0) and all(errors <= compared)
    assert ref.equivalent(c["code"], c["hypotheses"][best], c["truth"])


def test_shape_cases_reach_every_way_of_reading_a_row():
    assert {r for _, r in ref.SHAPE_CASES} == {"0 mod 16", "8 mod 16", "4 mod 8", "2 mod 4", "odd"}
    cases = [ref.make_case(n) for n, _ in ref.SHAPE_CASES]
    last = {(c["decode_type"], c["code"].R, (c["T"] - c["head"] - c["tail"]) % c["W"] == 1) for c in cases}
    assert len(last) == 6                                              # every width with a remainder of 1 step and of W - 1


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
