"""The rule of vit_hip_frames_extract on the host (no GPU): frame_sync.frames_extract_numpy against the two restatements of
tests/frames_reference.py on random shapes, cut invariance, a re-lock between two calls, the CCSDS randomiser, and the receiver's
composition of search, lock and extraction."""
import numpy as np
import pytest

from viterbidecodercpp_amd import CCSDS_ASM, frame_sync
from tests import frames_reference as fr


def random_shape(rng):
    P = int(rng.choice([8, 9, 13, 64, 67, 83, 200, int(rng.integers(8, 400))]))
    n_bits = int(rng.choice([1, P - 1, P, 3 * P + 5, int(rng.integers(1, 6 * P))]))
    c = int(rng.choice([0, 1, 7, 8, 9, P - 1, P, P + 50, int(rng.integers(0, P))]))
    d = int(rng.choice([0, 5, 32, int(rng.integers(0, P))])) % P
    m = min(int(rng.choice([0, 1, 8, 32, 64])), P)
    return dict(rows=1, n_bits=n_bits, P=P, phase0=int(rng.integers(0, P)), c=c, d=d, m=m, inverted=int(rng.integers(0, 2)),
                skip=[None, 0, 1, P - 1][int(rng.integers(0, 4))], pad=bool(rng.integers(0, 2)), carry=bool(rng.integers(0, 4)),
                phase_plus=P * int(rng.integers(0, 3)))


def test_the_restatements_agree_on_random_shapes():
    rng = np.random.default_rng(2026)
    seen_empty = seen_full = 0
    for i in range(300):
        c = fr.make_case(i, **random_shape(rng))
        loop, ints = fr.case_reference(c, fr.extract_loop)[0], fr.case_reference(c, fr.extract_ints)[0]
        got = frame_sync.frames_extract_numpy(c["bytes"][0], c["n_bits"], c["P"], c["phase0"], c["lock"][0], None if c["carry"] is None
                                              else c["carry"][0], int(c["carry_bits"][0]), c["marker"], c["m"], c["d"], c["pad"])
        for other in (loop, ints):
            assert np.array_equal(got[0], other[0]) and np.array_equal(got[2], other[2]) and got[3] == other[3], (i, c["P"], c["n_bits"])
            assert (got[1] is None and other[1] is None) or list(got[1]) == list(other[1]), i
        assert len(got[0]) <= fr.capacity(c["n_bits"], c["P"]) and got[0].shape[1] == c["qb"]
        seen_empty += len(got[0]) == 0
        seen_full += len(got[0]) >= 3
    assert seen_empty > 20 and seen_full > 20


def run_calls(bits, cuts, P, phase, inverted, marker, m, d, pad, form=None):
    """the stream `bits` in calls of `cuts` bits each, the carry handed from call to call: (frames, errors, last carry, its bits)"""
    frames, errors, carry, cbits, at = [], [], None, 0, 0
    for n in cuts:
        row = np.packbits(bits[at:at + n])
        if form is None:
            out = frame_sync.frames_extract_numpy(row, n, P, at % P, (phase, inverted), carry, cbits, marker, m, d, pad)
        else:
            out = form(row, n, P, at % P, phase, inverted, carry, cbits, marker, m, d, pad)
        frames += list(out[0])
        errors += list(out[1])
        carry, cbits = out[2], out[3]
        at += n
    return np.array(frames, dtype=np.uint8), np.array(errors), carry, cbits


@pytest.mark.parametrize("P,d,m", [(67, 5, 8), (288, 32, 32), (13, 0, 13), (1632, 8, 8)])
def test_cut_invariance(P, d, m):
    """one stream cut into calls at random bit lengths -- some shorter than P, several in a row, so that a frame spans three or more
    calls and calls complete nothing -- yields the frames, distances and final carry of ONE call"""
    rng = np.random.default_rng(P)
    bits = rng.integers(0, 2, size=9 * P + 11, dtype=np.uint8)
    pad = rng.integers(0, 256, size=(P - d + 7) // 8, dtype=np.uint8)
    marker = int(rng.integers(0, 1 << min(m, 62)))
    phase, inverted = int(rng.integers(0, P)), 1
    whole = run_calls(bits, [bits.size], P, phase, inverted, marker, m, d, pad)
    assert len(whole[0]) in (8, 9)
    for trial in range(6):
        small = [int(x) for x in rng.integers(1, max(P // 3, 2), size=7)]                 # a frame spans more than three of these
        rest = bits.size - sum(small)
        inner = np.sort(rng.choice(np.arange(1, rest), size=4, replace=False))
        cuts = small + [int(x) for x in np.diff(np.concatenate([[0], inner, [rest]]))]
        assert sum(cuts) == bits.size
        for form in (None, fr.extract_loop if P < 300 else fr.extract_ints):
            got = run_calls(bits, cuts, P, phase, inverted, marker, m, d, pad, form)
            assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), (trial, cuts)
            assert np.array_equal(got[2], whole[2]) and got[3] == whole[3]
    # and calls that complete nothing exist among them
    out = frame_sync.frames_extract_numpy(np.packbits(bits[:P // 3]), P // 3, P, 0, (phase, inverted), None, 0, marker, m, d, pad)
    assert len(out[0]) == 0


def test_a_changed_lock_phase_drops_exactly_the_stale_partial_frame():
    P, rng = 64, np.random.default_rng(3)
    bits = rng.integers(0, 2, size=400, dtype=np.uint8)
    # call 1 under phase 10: frames start at 10, 74, 138; bits [138, 170) are carried
    f1, _, carry, cbits = frame_sync.frames_extract_numpy(np.packbits(bits[:170]), 170, P, 0, (10, 0))
    assert len(f1) == 2 and cbits == 32 and np.array_equal(np.unpackbits(carry)[:32], bits[138:170])
    # call 2 under the same lock completes the carried frame ...
    same, _, _, _ = frame_sync.frames_extract_numpy(np.packbits(bits[170:]), 230, P, 170 % P, (10, 0), carry, cbits)
    assert np.array_equal(np.unpackbits(same[0]), bits[138:202])
    # ... and under phase 30 it drops the 32 carried bits and the 20 in front of the new start at 158 + 64 k: the next start is 222
    moved, _, carry2, cbits2 = frame_sync.frames_extract_numpy(np.packbits(bits[170:]), 230, P, 170 % P, (30, 0), carry, cbits)
    starts = [158 + 64 * k for k in range(4)]                       # 158 lies inside the carry: the frame from 158 is whole in S
    assert len(moved) == 3 and [np.array_equal(np.unpackbits(moved[k]), bits[s:s + 64]) for k, s in enumerate(starts[:3])] == [True] * 3
    assert cbits2 == 400 - 350 and np.array_equal(np.unpackbits(carry2)[:cbits2], bits[350:])
    for form in (fr.extract_loop, fr.extract_ints):
        other = form(np.packbits(bits[170:]), 230, P, 170 % P, 30, 0, carry, cbits)
        assert np.array_equal(other[0], moved) and other[3] == cbits2


def test_ccsds_randomizer():
    assert frame_sync.ccsds_randomizer(8).tobytes() == bytes.fromhex("FF480EC09A0D70BC")
    bits = np.unpackbits(frame_sync.ccsds_randomizer(255))
    assert np.array_equal(bits[:255 * 7], bits[255:])
    assert not any(np.array_equal(bits[:255], bits[p:p + 255]) for p in range(1, 255))
    assert frame_sync.ccsds_randomizer(0).size == 0


def test_rejections():
    row = np.zeros(16, dtype=np.uint8)
    for kw in (dict(period=7), dict(phase0=64), dict(drop_bits=64), dict(n_bits=0), dict(n_bits=129), dict(marker_bits=65),
               dict(marker=0x100, marker_bits=8)):
        args = dict(row=row, n_bits=128, period=64, phase0=0, lock=(0, 0)) | kw
        with pytest.raises(ValueError):
            frame_sync.frames_extract_numpy(**args)


RECEIVER = dict(P=288, d=32, lead=20, n_frames=12, trail=64)     # the trail keeps a decoder's end effects out of the last frame
FIRST_GOOD_FRAME = 0           # a call that completes a frame has emitted 288 bits, the first marker among them: the lock is right
LATE_LEAD, LATE_CHUNKS, LATE_FIRST_GOOD = 20 + 2 * 288, [10, 300, 7, 290, 100, 500, 31, 1000], 1


def test_receiver_composition_returns_the_transmitted_frames():
    P, d = RECEIVER["P"], RECEIVER["d"]
    pad = frame_sync.ccsds_randomizer((P - d) // 8)
    bits, payload = fr.framed_stream(77, *CCSDS_ASM, P, RECEIVER["n_frames"], RECEIVER["lead"], pad, RECEIVER["trail"])
    for chunks in ([bits.size], [64, 64, 200, 1, 31, 500, 333], [10, 300, 700]):
        chunks = chunks + [bits.size - sum(chunks)] if sum(chunks) < bits.size else chunks
        for inverted in (0, 1):
            frames, errors, locks = fr.receiver_numpy(bits ^ np.uint8(inverted), chunks, *CCSDS_ASM, P, d, pad)
            good = next(i for i, lk in enumerate(locks) if lk == (RECEIVER["lead"], inverted))
            assert good == FIRST_GOOD_FRAME and len(frames) == RECEIVER["n_frames"]
            assert np.array_equal(frames[good:], payload) and not errors[good:].any()
    # two periods of noise in front of the first marker: calls complete frames before the marker has been seen
    bits, payload = fr.framed_stream(78, *CCSDS_ASM, P, 8, LATE_LEAD, pad)
    chunks = LATE_CHUNKS + [bits.size - sum(LATE_CHUNKS)]
    frames, errors, locks = fr.receiver_numpy(bits, chunks, *CCSDS_ASM, P, d, pad)
    good = next(i for i, lk in enumerate(locks) if lk == (20, 0))
    assert good == LATE_FIRST_GOOD, (good, locks)
    assert all(lk == (20, 0) for lk in locks[good:]) and errors[:good].all() and not errors[good:].any()
    assert np.array_equal(frames[good:], payload[len(payload) - (len(frames) - good):])
