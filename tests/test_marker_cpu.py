"""Frame synchronisation on the CPU: the rule of vit_hip_marker_search written three times (tests/marker_reference.py twice,
viterbidecodercpp_amd.frame_sync once) agrees with itself; the pick on hand-made totals; the marker names the true phase and polarity
of decoded Voyager frames; a stream searched piecewise with history sums to one search; and the surface the layers export."""
import os
import subprocess

import numpy as np
import pytest

from tests import marker_reference as mr
from tests import stream_reference as sr
from tests.helpers import oracle_cfg
from viterbidecodercpp_amd import CCSDS_ASM, COMMON_CODES, DVB_SYNC, _lib, frame_sync, get_decoding_config, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_shape(rng):
    m = int(rng.choice([1, 7, 8, 9, 31, 32, 33, 63, 64, int(rng.integers(1, 65))]))
    hb = int(rng.choice([0, 1, m - 1, 63, int(rng.integers(0, 64))]))
    n_bits = int(rng.choice([0, m, m + 1, int(rng.integers(0, 400))]))
    if n_bits + hb < m:
        n_bits = m - hb
    P = int(rng.choice([1, max(m - 1, 1), 8, 13, n_bits + 5, int(rng.integers(1, 200))]))
    return dict(rows=int(rng.integers(1, 4)), n_bits=n_bits, m=m, P=P, hb=hb, phase0=int(rng.integers(0, P)))


def test_the_three_forms_agree():
    rng = np.random.default_rng(7)
    for i in range(120):
        c = mr.make_case(1000 + i, **_random_shape(rng), stride_extra=int(rng.integers(0, 3)))
        args = (c["bytes"][:, :c["nb"]], c["n_bits"], c["marker"], c["m"], c["P"], c["phase0"], c["history"], c["hb"])
        loop, fast, lib = mr.search_loop(*args), mr.search_fast(*args), frame_sync.marker_search_numpy(*args)
        for got in (fast, lib):
            assert np.array_equal(got[0], loop[0]) and np.array_equal(got[1], loop[1]), (i, c["n_bits"], c["m"], c["P"], c["hb"])
        assert loop[1].sum() == c["rows"] * (c["n_bits"] + c["hb"] - c["m"] + 1)
        want = mr.pick_loop(*loop, c["m"])
        assert np.array_equal(mr.pick(*loop, c["m"]), want) and np.array_equal(frame_sync.marker_lock_numpy(*loop, c["m"]), want)


# distance [P], count [P], m -> (phase, inverted, errors, compared)
_M = 1 << 31
PICKS = [
    ("equal rates, other denominators: the lower phase", [3, 1, 2], [6, 2, 4], 1, (0, 0, 3, 6)),
    ("equal rates behind a worse one", [4, 2, 1], [6, 4, 2], 1, (0, 1, 2, 6)),                   # 4/6 upright, 2/6 inverted at phase 0
    ("products above 2^32, low halves the other way", [mr.WRAP_ERRORS + 1, mr.WRAP_ERRORS], [mr.WRAP_COMPARED, mr.WRAP_COMPARED], 1,
     (1, 0, mr.WRAP_ERRORS, mr.WRAP_COMPARED)),
    ("products 2^32 apart", [1_500_000_002, 1_500_000_000], [_M, _M], 1, (0, 1, _M - 1_500_000_002, _M)),
    ("phases of count 0 in front", [0, 0, 5, 4], [0, 0, 1, 1], 32, (3, 0, 4, 32)),
    ("nothing compared anywhere", [0, 0, 0], [0, 0, 0], 8, (0, 0, 0, 0)),
    ("a tie between phases", [9, 3, 3, 9], [4, 4, 4, 4], 8, (1, 0, 3, 32)),
    ("upright and inverted tie, other denominators", [8, 4], [2, 1], 8, (0, 0, 8, 16)),
    ("upright and inverted tie at half", [4, 4], [1, 1], 8, (0, 0, 4, 8)),
    ("inverted wins", [30, 16], [1, 1], 32, (0, 1, 2, 32)),
    ("an inverted phase ties with a later upright one", [29, 3], [1, 1], 32, (0, 1, 3, 32)),
]


@pytest.mark.parametrize("name,distance,count,m,want", PICKS, ids=[p[0] for p in PICKS])
def test_pick_on_hand_made_totals(name, distance, count, m, want):
    for form in (mr.pick, mr.pick_loop, frame_sync.marker_lock_numpy):
        assert tuple(int(x) for x in form(distance, count, m)[0]) == want, form.__name__


def test_the_low_halves_of_the_wrapped_products_order_the_other_way():
    ea, ca, eb, cb = mr.WRAP_ERRORS, mr.WRAP_COMPARED, mr.WRAP_ERRORS + 1, mr.WRAP_COMPARED
    assert ea * cb > 1 << 32 and 2 * ea < ca                     # upright: the inverted candidates are far worse
    assert mr.beats(ea, ca, eb, cb) and not (ea * cb) & 0xFFFFFFFF < (eb * ca) & 0xFFFFFFFF


TRUTH_SEED, TRUTH_PHASE, TRUTH_PERIOD, TRUTH_FRAMES = 1, 300, 1024, 8


def test_the_marker_names_the_true_phase_and_polarity(oracle):
    """Voyager SOFT16 at 4 dB, 8 frames of 1024 bits with the CCSDS marker at phase 300, decoded by the oracle as one stream: the
    lock names phase 300 upright; on the negated symbols (a transparent code: the decoded bits are inverted) the same phase
    inverted, with the same errors.  On the oracle the winner's rate is 0 / 256 and the runner-up's 92 / 256 = 0.359."""
    code = COMMON_CODES[2]
    pc = get_decoding_config("SOFT16", code.R)
    bits = mr.frames_with_marker(TRUTH_SEED, *CCSDS_ASM, TRUTH_PERIOD, TRUTH_FRAMES, TRUTH_PHASE)
    coded = synth.encode_bits_numpy(code.K, code.R, code.G, np.packbits(bits)[None])
    sym = synth.quantise_numpy(coded, pc.soft_decision_high, pc.soft_decision_low, 4.0, code.R, np.random.default_rng(TRUTH_SEED + 100),
                               pc.soft_dtype)[0]
    negated = (pc.soft_decision_high + pc.soft_decision_low - sym.astype(np.int64)).astype(sym.dtype)
    locks = []
    for s in (sym, negated):
        by, n = sr.stream_reference(oracle, code, oracle_cfg("SOFT16", code.R), s, 1024, flags=sr.BEGIN | sr.END)
        assert n == bits.size
        d, c = frame_sync.marker_search_numpy(by, n, *CCSDS_ASM, TRUTH_PERIOD)
        locks.append(tuple(int(x) for x in mr.pick(d, c, CCSDS_ASM[1])[0]))
    assert locks[0][:2] == (TRUTH_PHASE, 0) and locks[1][:2] == (TRUTH_PHASE, 1)
    assert locks[0][2:] == locks[1][2:] and locks[0][3] == 32 * TRUTH_FRAMES


@pytest.mark.parametrize("marker,P", [(CCSDS_ASM, 1024), (DVB_SYNC, 1632), ((0x5, 3), 7), ((0x9D3C5A7E12345678, 64), 200)])
def test_chunked_totals_sum_to_one_search(marker, P):
    """a bit stream cut at random places -- cuts shorter than the marker, cuts inside a marker -- searched piecewise with the last m-1
    bits as history and the bits so far mod P as phase0"""
    value, m = marker
    rng = np.random.default_rng(m * 1000 + P)
    bits = mr.frames_with_marker(int(rng.integers(1 << 30)), value, m, P, 0, phase=int(rng.integers(P)), n_bits=5 * P + 37)
    want = mr.search_fast(np.packbits(bits), bits.size, value, m, P)
    cuts = sorted(set(int(x) for x in rng.integers(0, bits.size, size=12)) | {3, 3 + max(m - 2, 1)})
    marker_at = next(p for p in range(bits.size) if p > cuts[2] and np.array_equal(bits[p:p + m], mr.marker_bits_of(value, m)))
    cuts = sorted(set(cuts) | {marker_at + m // 2}) + [bits.size]
    distance, count, done, searched, skipped = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64), 0, 0, 0
    for cut in cuts:
        piece = bits[done:cut]
        word, hb = frame_sync.history_of(bits[:done], m)
        if piece.size + hb >= m:
            d, c = frame_sync.marker_search_numpy(np.packbits(piece), piece.size, value, m, P, done % P, [word], hb)
            distance += d[0]
            count += c[0]
            searched += 1
        else:
            skipped += 1                      # the piece only extends the history
        done = cut
    assert np.array_equal(distance, want[0][0]) and np.array_equal(count, want[1][0])
    assert searched >= 3 and (m < 8 or skipped >= 1)


def test_marker_surface():
    assert "vit_hip_marker_search" in _lib.EXPORTS and _lib.MARKER_ACCUMULATE == 1
    lib = _lib.load()
    assert len(lib.vit_hip_marker_search.argtypes) == 16
    import viterbidecodercpp_amd
    from viterbidecodercpp_amd import BatchDecoder, MultiStreamDecoder
    for name in ("CCSDS_ASM", "DVB_SYNC", "marker_search_numpy"):
        assert name in viterbidecodercpp_amd.__all__
    assert CCSDS_ASM == (0x1ACFFC1D, 32) and DVB_SYNC == (0x47, 8)
    assert callable(BatchDecoder.marker_search)
    assert isinstance(MultiStreamDecoder.marker_totals, property) and isinstance(MultiStreamDecoder.marker_lock, property)
    kernels = _lib.list_kernels()
    assert any("marker_search_kernel" in k for k in kernels) and any("marker_pick_kernel" in k for k in kernels)
    for name, r in kernels.items():
        if "marker_" in name:
            assert r["scratch_bytes"] == 0, (name, r)


def test_marker_rejections_need_no_gpu():
    """the argument rule is checked before the device is touched: a NULL handle and every rejection return INVALID_ARG"""
    lib = _lib.load()
    assert lib.vit_hip_marker_search(None, None, 0, 1, 64, 0x47, 8, None, 0, 8, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert b"NULL handle" in lib.vit_hip_last_error()


def test_marker_cpp_surface(tmp_path):
    src = tmp_path / "marker.cpp"
    src.write_text(
        '#include "viterbi_hip/viterbi_decoder_hip_batch.h"\n'
        "void f(ViterbiDecoder_HIP_Batch<7, 2, uint16_t, int16_t>& d, const uint8_t* bytes, const uint64_t* history, uint32_t* distance,\n"
        "       uint32_t* count, vit_hip_marker_lock* lock) {\n"
        "    d.marker_search(bytes, 1, size_t(1) << 26, 0x1ACFFC1D, 32, 10232, distance);\n"
        "    d.marker_search(bytes, 64, 16384, 0x47, 8, 1632, distance, count, lock, 5, history, 7, VIT_HIP_MARKER_ACCUMULATE, 2064, nullptr);\n"
        "    (void)(lock->phase + lock->inverted + lock->errors + lock->compared);\n"
        "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
