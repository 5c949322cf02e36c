"""The Reed-Solomon cases the CPU and the GPU tests share: codes, shapes, error patterns and -- computed once per case by
tests/rs_reference.py -- what the rule makes of them.  tests/test_rs_cpu.py checks the seeds (every codeword with more than t errors
must come back -1 from the reference where t >= 8) so that a wrong seed fails there, not on the GPU."""
import functools

import numpy as np

from viterbidecodercpp_amd.reed_solomon import (CCSDS_RS_255_223, CCSDS_RS_255_223_DUAL, CCSDS_RS_255_239, CCSDS_RS_255_239_DUAL,
                                                DVB_RS_204_188, RSCode, rs_encode_numpy)
from tests import rs_reference as ref

CODES = {
    "ccsds223": CCSDS_RS_255_223, "ccsds223dual": CCSDS_RS_255_223_DUAL, "ccsds239": CCSDS_RS_255_239, "ccsds239dual": CCSDS_RS_255_239_DUAL,
    "dvb": DVB_RS_204_188, "nroots2": RSCode(0x11D, 1, 1, 2), "nroots64": RSCode(0x187, 96, 11, 64),
    "short": RSCode(0x187, 112, 11, 32, pad=100), "nroots3": RSCode(0x187, 5, 7, 3),
}
# (code, interleave, rows, max_frames): every depth of {1, 2, 5, 8} and every batch of {1x1, 3x2, 2x5}, each code in a case whose plain frames hold at
# least 7 codewords; depth 11 takes the kernel's second tile of codewords
SHAPES = [("ccsds223dual", 5, 2, 5), ("ccsds223", 2, 2, 5), ("ccsds239", 8, 3, 2), ("ccsds239dual", 2, 2, 5), ("dvb", 5, 3, 2),
          ("nroots2", 8, 2, 5), ("nroots64", 5, 3, 2), ("short", 5, 3, 2), ("nroots3", 8, 3, 2), ("ccsds223dual", 1, 1, 1), ("dvb", 1, 2, 5),
          ("nroots2", 1, 3, 2), ("dvb", 2, 3, 2), ("short", 8, 1, 1), ("ccsds223", 11, 1, 1)]
PLACES = ("any", "first", "last", "parity", "data")


def error_counts(code):
    t = code.t
    return [0, 1, max(t - 1, 0), t, t + 1, t + 5, 200]


@functools.lru_cache(maxsize=None)
def make_case(name, I, rows, max_frames, seed=0):
    """frames uint8 [rows][max_frames][n I] with, codeword after codeword, 0, 1, t-1, t, t+1, t+5 and 200 byte errors (a clean one
    between bad ones), placed anywhere, from position 0 on, from position n-1 back, in the parity or in the data; one frame carries a
    burst of I t consecutive bytes instead, one the all-zero and one the all-0xFF word.  returns a dict with the sent frames, the
    received ones, the error count of every codeword and the reference's (frames, status)."""
    code = ALL_CODES[name]
    rng = np.random.default_rng([seed, I, rows, max_frames, code.nroots, code.pad])
    n, k, t = code.n, code.k, code.t
    data = rng.integers(0, 256, size=(rows, max_frames, k * I), dtype=np.uint8)
    sent = rs_encode_numpy(code, data, I)
    got = sent.copy()
    counts = np.zeros((rows, max_frames, I), dtype=np.int64)
    menu = error_counts(code)
    idx = seed
    flat, cflat = got.reshape(-1, n * I), counts.reshape(-1, I)
    for m in range(flat.shape[0]):
        for c in range(I):
            count = min(menu[idx % len(menu)], n)
            place = PLACES[(idx // len(menu)) % len(PLACES)]
            if (place == "parity" and count > code.nroots) or (place == "data" and count > k) or count >= n:
                place = "any"
            ref.corrupt(rng, flat[m], I, c, count, place, n, code.nroots)
            cflat[m, c] = count
            idx += 1
    if flat.shape[0] >= 4:
        flat[1] = sent.reshape(-1, n * I)[1]                       # a burst of I t bytes: t errors in every codeword
        start = int(rng.integers(0, n * I - I * t + 1))
        flat[1, start:start + I * t] ^= rng.integers(1, 256, size=I * t).astype(np.uint8)
        cflat[1] = t
        flat[2], cflat[2] = 0x00, -2                               # not what was sent: whatever the rule says of them
        flat[3], cflat[3] = 0xFF, -2
    want, status = ref.decode(code, got, I)
    return dict(code=code, I=I, rows=rows, max_frames=max_frames, sent=sent, got=got, counts=counts, want=want, status=status)


def check_seed(case):
    """what the error counts promise, said by the reference alone"""
    code, counts, status = case["code"], case["counts"], case["status"]
    known = counts >= 0
    assert np.array_equal(status[known & (counts <= code.t)], counts[known & (counts <= code.t)])
    ok = (status >= 0) & known
    assert np.array_equal(case["want"].reshape(-1, code.n, case["I"]).transpose(0, 2, 1)[ok.reshape(-1, case["I"])],
                          case["sent"].reshape(-1, code.n, case["I"]).transpose(0, 2, 1)[ok.reshape(-1, case["I"])]) or code.t < 8
    if code.t >= 8:                                               # a miscorrection has probability about 1 / t!
        assert (status[known & (counts > code.t)] == -1).all()


# ---- the second pass: the codes, depths and words the batches above never reach.  SHAPES and CODES above stay as they are.
# Together with CODES: all 16 primitive polynomials of degree 8, fcr 0 and 254, prim 254 and eleven more values outside {1, 7, 11},
# nroots 4, 5, 6, 8, 9, 17, 33 (R2 = 4, 8, 16, 32, 64 from just above the power of two below), n = nroots + 1 for nroots 2, 9, 33
# and 64, n = 252 with one segment (no zero fill at all) and n % 4 = 1, 2, 3 with one segment
PRIMITIVE_POLYNOMIALS = (0x11D, 0x12B, 0x12D, 0x14D, 0x15F, 0x163, 0x165, 0x169, 0x171, 0x187, 0x18D, 0x1A9, 0x1C3, 0x1CF, 0x1E7, 0x1F5)
NEW_CODES = {
    "n2k1": RSCode(0x11D, 1, 1, 2, pad=252), "n4": RSCode(0x12B, 0, 2, 4), "n5": RSCode(0x12D, 0, 2, 5), "n6": RSCode(0x169, 3, 4, 6),
    "n8": RSCode(0x14D, 254, 254, 8, pad=30), "n9k1": RSCode(0x15F, 1, 13, 9, pad=245), "n17": RSCode(0x163, 7, 19, 17, pad=3),
    "n33": RSCode(0x165, 200, 1, 33, pad=3), "n33k1": RSCode(0x165, 200, 1, 33, pad=221), "n33a": RSCode(0x171, 5, 14, 33, pad=2),
    "n33b": RSCode(0x18D, 100, 23, 33, pad=1), "n33c": RSCode(0x1A9, 253, 253, 33), "n64k1": RSCode(0x1F5, 0, 7, 64, pad=190),
    "p1c3": RSCode(0x1C3, 9, 8, 4, pad=215), "p1cf": RSCode(0x1CF, 77, 16, 4, pad=215), "p1e7": RSCode(0x1E7, 130, 29, 4, pad=215),
}
ALL_CODES = {**CODES, **NEW_CODES}  # CODES itself stays: every code in it must see the whole error menu within SHAPES

# make_case(name, I, 3, 2) for every new code, and the k = 1 codes once more with one codeword per frame
GEOMETRY = ([(name, 5 if code.n <= 40 else 2, 3, 2) for name, code in NEW_CODES.items()]
            + [(name, 1, 3, 2) for name in ("n2k1", "n9k1", "n33k1", "n64k1")])
SWEEPS = ["ccsds223dual", "dvb", "nroots64", "n5", "n8", "n17", "n33"]
DESIGNED = [("ccsds223", ("lead", "trail")), ("dvb", ("lead", "trail", "fill")), ("n8", ("lead", "trail", "fill")),
            ("n17", ("lead", "trail", "fill")), ("short", ("fill",))]
MISCORRECTING = ["n4", "n6"]
# more than one tile of 8 codewords together with more than one frame: one codeword in the last tile (9, 17), full tiles only (16, 64)
TILED = [(name, I, 2, 3) for name in ("dvb", "n8") for I in (9, 16, 17, 64)] + [(name, 11, 3, 2) for name in ("dvb", "n8")]
TINY = [("n2k1", I, 3, 2) for I in (1, 2, 3)]                    # frames of 3, 6 and 9 bytes
DWORDS = [(name, I, 3, 2) for name in ("ccsds239", "n33a") for I in (8, 4)]


def _case(code, I, sent, got, counts, **more):
    want, status = ref.decode(code, got, I)
    rows, max_frames = got.shape[:2]
    return dict(code=code, I=I, rows=rows, max_frames=max_frames, sent=sent, got=got, counts=counts, want=want, status=status, **more)


@functools.lru_cache(maxsize=None)
def make_sweep(name):
    """I = 1, one row of t + 3 frames: frame e carries exactly e byte errors at random places, e = 0 .. t + 2"""
    code = ALL_CODES[name]
    rng = np.random.default_rng([7, code.nroots, code.pad, code.gfpoly])
    frames = code.t + 3
    sent = rs_encode_numpy(code, rng.integers(0, 256, size=(1, frames, code.k), dtype=np.uint8))
    got = sent.copy()
    for e in range(frames):
        ref.corrupt(rng, got[0, e], 1, 0, e)
    return _case(code, 1, sent, got, np.arange(frames, dtype=np.int64).reshape(1, frames, 1))


def root_product(code, js):
    """the coefficients, low to high, of the product of (x - root_j) over j in js: len(js) + 1 of them, none zero (it generates an
    MDS code); by the reference's roots and product table alone"""
    M, rts = ref.mul_table(code.gfpoly), ref.roots(code.gfpoly, code.fcr, code.prim, code.nroots)
    poly = [1]
    for j in js:
        poly = [(poly[i - 1] if i else 0) ^ (int(M[poly[i], rts[j]]) if i < len(poly) else 0) for i in range(len(poly) + 1)]
    return poly


def zero_run_lengths(code):
    t = code.t
    return sorted({m for m in (1, 2, t // 2, t - 1, t, t + 4) if 1 <= m < code.nroots})


@functools.lru_cache(maxsize=None)
def make_designed(name, kinds=("lead", "trail", "fill")):
    """I = 1, one row of frames made to order; case["kinds"][f] says what frame f is:
      ("lead", m)      the error is a scalar multiple of x^off prod_(j < m) (x - root_j): m + 1 wrong bytes whose syndromes S_0 .. S_(m-1)
                       vanish and S_m does not, so Berlekamp-Massey keeps L = 0 through m steps and jumps to m + 1.  m + 1 <= t is
                       corrected; above that no word of weight <= t has these syndromes (t vanishing syndromes in a row and at most t
                       errors mean no error), so the rule says -1
      ("trail", m)     the same with the roots nroots - m .. nroots - 1: the last m discrepancies are zero
      ("fill", w, x)   (pad > 0) a codeword of the parent code (pad = 0) whose virtual fill holds w non-zero bytes, the transmitted n
                       bytes of it with x further errors, w + x <= t: the only codeword within t has a non-zero fill, every other one
                       is at least nroots + 1 - t > t away, so the locator's roots are all found, w of them at p >= n: -1, unchanged"""
    code = ALL_CODES[name]
    assert not code.dual_basis
    M = ref.mul_table(code.gfpoly)
    n, k, t, nroots = code.n, code.k, code.t, code.nroots
    rng = np.random.default_rng([11, nroots, code.pad, code.gfpoly])
    sent, got, what, counts = [], [], [], []
    for kind in kinds:
        if kind == "fill":
            assert code.pad > 0
            parent = RSCode(code.gfpoly, code.fcr, code.prim, nroots)
            for w in sorted({1, min(t, code.pad)}):
                for x in sorted({0, t - w}):
                    data = rng.integers(0, 256, size=parent.k, dtype=np.uint8)
                    data[:code.pad] = 0
                    data[rng.choice(code.pad, size=w, replace=False)] = rng.integers(1, 256, size=w)
                    word = rs_encode_numpy(parent, data[None])[0, code.pad:]
                    sent.append(word)
                    got.append(word.copy())
                    ref.corrupt(rng, got[-1], 1, 0, x)
                    what.append(("fill", w, x))
                    counts.append(-2)                               # not a codeword of this code was sent
            continue
        for m in zero_run_lengths(code):
            poly = root_product(code, range(m) if kind == "lead" else range(nroots - m, nroots))
            scale, off = int(rng.integers(1, 256)), int(rng.integers(0, n - m))
            word = rs_encode_numpy(code, rng.integers(0, 256, size=(1, k), dtype=np.uint8))[0]
            sent.append(word)
            got.append(word.copy())
            for i, coeff in enumerate(poly):                        # the coefficient of x^p is byte n - 1 - p
                got[-1][n - 1 - (off + i)] ^= int(M[coeff, scale])
            what.append((kind, m))
            counts.append(m + 1)
    frames = len(sent)
    return _case(code, 1, np.array(sent).reshape(1, frames, n), np.array(got).reshape(1, frames, n),
                 np.array(counts, dtype=np.int64).reshape(1, frames, 1), kinds=what)


@functools.lru_cache(maxsize=None)
def make_miscorrecting(name, words=300):
    """I = 1, one row of `words` codewords with t + 1, t + 2, t + 3 errors in turn: at t = 2 and 3 another codeword often lies within t
    of such a word, and a bounded-distance decoder must then move to it"""
    code = ALL_CODES[name]
    rng = np.random.default_rng([13, code.nroots, code.pad, code.gfpoly])
    sent = rs_encode_numpy(code, rng.integers(0, 256, size=(1, words, code.k), dtype=np.uint8))
    got = sent.copy()
    counts = (code.t + 1 + np.arange(words) % 3).reshape(1, words, 1).astype(np.int64)
    for m in range(words):
        ref.corrupt(rng, got[0, m], 1, 0, int(counts[0, m, 0]))
    return _case(code, 1, sent, got, counts)


def make_tiled(name, I, rows, max_frames):
    """make_case under another seed: the error menu starts one entry on"""
    return make_case(name, I, rows, max_frames, seed=1)


@functools.lru_cache(maxsize=None)
def make_many(rows=2, max_frames=35000, distinct=512):
    """`distinct` different frames of the (3, 1) code -- clean words, a single error at each of the three positions, double errors --
    decoded once by the reference and repeated to rows x max_frames frames: the rule treats every codeword on its own, so the
    repeated answers are the reference's answer.  70 000 blocks of one wave each.  case["base"] is the case of the distinct frames."""
    code = ALL_CODES["n2k1"]
    rng = np.random.default_rng(17)
    seen, sent, got, counts = set(), [], [], []
    while len(got) < distinct:
        kind = len(got) % 5                                         # clean, an error at position 0, 1, 2, two errors
        word = rs_encode_numpy(code, rng.integers(0, 256, size=(1, code.k), dtype=np.uint8))[0]
        bad = word.copy()
        for pos in ([], [0], [1], [2], rng.choice(3, size=2, replace=False).tolist())[kind]:
            bad[pos] ^= int(rng.integers(1, 256))
        if bad.tobytes() not in seen:
            seen.add(bad.tobytes())
            sent.append(word)
            got.append(bad)
            counts.append(min(kind, 1) if kind < 4 else 2)
    base = _case(code, 1, np.array(sent)[None], np.array(got)[None], np.array(counts, dtype=np.int64).reshape(1, distinct, 1))
    reps = -(-rows * max_frames // distinct)

    def repeat(x):
        return np.tile(x[0], (reps, 1))[:rows * max_frames].reshape(rows, max_frames, x.shape[-1])

    return dict(code=code, I=1, rows=rows, max_frames=max_frames, base=base,
                **{key: repeat(base[key]) for key in ("sent", "got", "counts", "want", "status")})
