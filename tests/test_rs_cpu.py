"""viterbidecodercpp_amd.reed_solomon without a GPU: constants computed outside any decoder, the encoder, and the package's rule
(Berlekamp-Massey, root search, Forney) against tests/rs_reference.py (a product table, Peterson-Gorenstein-Zierler, the answer
checked by definition) byte for byte -- over the cases the GPU tests use, whose seeds are checked here."""
import numpy as np
import pytest

from viterbidecodercpp_amd import reed_solomon as rs
from viterbidecodercpp_amd import CCSDS_RS_255_223, CCSDS_RS_255_223_DUAL, CCSDS_RS_255_239, CCSDS_RS_255_239_DUAL, DVB_RS_204_188, RSCode
from tests import rs_cases, rs_reference as ref


def test_generator_polynomials():
    g = rs.generator(CCSDS_RS_255_223)
    assert len(g) == 33 and g == g[::-1] and list(g[:6]) == [0x01, 0x5B, 0x7F, 0x56, 0x10, 0x1E]
    assert list(rs.generator(DVB_RS_204_188)) == [59, 36, 50, 98, 229, 41, 65, 163, 8, 30, 209, 68, 189, 104, 13, 59, 1]
    assert (CCSDS_RS_255_239.fcr, CCSDS_RS_255_239.prim, CCSDS_RS_255_239.nroots) == (120, 11, 16)
    assert (DVB_RS_204_188.n, DVB_RS_204_188.k, DVB_RS_204_188.t) == (204, 188, 8)


def test_dual_basis_tables():
    to_dual, to_conv = rs.dual_basis_tables()
    assert to_dual[:10].tolist() == [0x00, 0x7B, 0xAF, 0xD4, 0x99, 0xE2, 0x36, 0x4D, 0xFA, 0x81]
    assert to_conv[:10].tolist() == [0x00, 0xCC, 0xAC, 0x60, 0x79, 0xB5, 0xD5, 0x19, 0xF0, 0x3C]
    assert sorted(to_dual.tolist()) == list(range(256)) and np.array_equal(to_conv[to_dual], np.arange(256))
    M = ref.mul_table(0x187)
    assert [ref.power(M, 2, e) for e in (125, 88, 226, 163, 46, 184, 67, 242)] == [int(to_conv[1 << (7 - i)]) for i in range(8)]
    other = ref.dual_tables(0x187)
    assert np.array_equal(other[0], to_dual) and np.array_equal(other[1], to_conv)


def test_parameters_are_checked():
    for bad in (dict(gfpoly=0x11B), dict(nroots=1), dict(nroots=65), dict(pad=230), dict(prim=3), dict(prim=0), dict(fcr=255),
                dict(gfpoly=0x87), dict(gfpoly=0x11D, dual_basis=True)):
        with pytest.raises(ValueError):
            RSCode(**{**dict(gfpoly=0x187, fcr=112, prim=11, nroots=32), **bad})


@pytest.mark.parametrize("code", [CCSDS_RS_255_223, CCSDS_RS_255_239, DVB_RS_204_188], ids=["223", "239", "dvb"])
def test_encoder_output_has_zero_syndromes(code):
    rng = np.random.default_rng(code.nroots)
    data = rng.integers(0, 256, size=(2, code.k * 3), dtype=np.uint8)
    frames = rs.rs_encode_numpy(code, data, 3)
    assert frames.shape == (2, code.n * 3)
    M, roots = ref.mul_table(code.gfpoly), ref.roots(code.gfpoly, code.fcr, code.prim, code.nroots)
    for f, d in zip(frames, data):
        for c in range(3):
            assert np.array_equal(f[c::3][:code.k], d[c::3]) and not ref.syndromes(M, roots, f[c::3]).any()
            assert not any(rs.syndromes(code, f[c::3]))


@pytest.mark.parametrize("conv,dual", [(CCSDS_RS_255_223, CCSDS_RS_255_223_DUAL), (CCSDS_RS_255_239, CCSDS_RS_255_239_DUAL)], ids=["223", "239"])
def test_dual_basis_encode_is_the_conventional_one_between_the_tables(conv, dual):
    to_dual, to_conv = rs.dual_basis_tables()
    data = np.random.default_rng(9).integers(0, 256, size=(2, conv.k * 2), dtype=np.uint8)
    assert np.array_equal(rs.rs_encode_numpy(dual, data, 2), to_dual[rs.rs_encode_numpy(conv, to_conv[data], 2)])


@pytest.mark.parametrize("shape", rs_cases.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_package_rule_equals_the_reference_on_the_shared_cases(shape):
    case = rs_cases.make_case(*shape)
    rs_cases.check_seed(case)
    frames, status = rs.rs_decode_numpy(case["code"], case["got"], case["I"])
    assert status.dtype == np.int32 and status.shape == case["status"].shape
    assert np.array_equal(status, case["status"]) and np.array_equal(frames, case["want"])


def test_the_cases_cover_what_they_promise():
    seen = {name: set() for name in rs_cases.CODES}
    for name, I, rows, max_frames in rs_cases.SHAPES:
        case = rs_cases.make_case(name, I, rows, max_frames)
        seen[name] |= set(case["counts"].reshape(-1).tolist())
    for name, code in rs_cases.CODES.items():
        assert set(min(c, code.n) for c in rs_cases.error_counts(code)) <= seen[name], name
    assert {s[1] for s in rs_cases.SHAPES} >= {1, 2, 5, 8} and {s[2:] for s in rs_cases.SHAPES} == {(1, 1), (3, 2), (2, 5)}


def test_random_codes_against_the_reference():
    rng = np.random.default_rng(2024)
    for _ in range(12):
        prim = int(rng.choice([p for p in range(1, 255) if np.gcd(p, 255) == 1]))
        nroots = int(rng.integers(2, 65))
        code = RSCode(int(rng.choice([0x187, 0x11D, 0x12B])), int(rng.integers(0, 255)), prim, nroots, int(rng.integers(0, 254 - nroots)))
        I = int(rng.integers(1, 4))
        got = rs.rs_encode_numpy(code, rng.integers(0, 256, size=(4, code.k * I), dtype=np.uint8), I)
        for m in range(4):
            for c in range(I):
                ref.corrupt(rng, got[m], I, c, min(int(rng.integers(0, code.t + 3)), code.n))
        want, status = ref.decode(code, got, I)
        frames, mine = rs.rs_decode_numpy(code, got, I)
        assert np.array_equal(mine, status) and np.array_equal(frames, want), code


def test_single_errors_of_a_two_root_code_exhaustively():
    code = RSCode(0x11D, 1, 1, 2)
    sent = rs.rs_encode_numpy(code, np.arange(code.k, dtype=np.uint8)[None])[0]
    got = np.repeat(sent[None], 255, axis=0)
    got[np.arange(255), np.arange(255)] ^= (1 + np.arange(255) % 255).astype(np.uint8)
    frames, status = rs.rs_decode_numpy(code, got)
    assert (status == 1).all() and (frames == sent).all()
    want, ref_status = ref.decode(code, got)
    assert np.array_equal(want, frames) and np.array_equal(ref_status, status)


def test_an_odd_number_of_roots():
    code = RSCode(0x187, 5, 7, 3, pad=200)                        # t = 1: the third syndrome only ever rejects
    rng = np.random.default_rng(3)
    sent = rs.rs_encode_numpy(code, rng.integers(0, 256, size=(40, code.k), dtype=np.uint8))
    got = sent.copy()
    for m in range(40):
        ref.corrupt(rng, got[m], 1, 0, m % 4)
    frames, status = rs.rs_decode_numpy(code, got)
    want, ref_status = ref.decode(code, got)
    assert np.array_equal(status, ref_status) and np.array_equal(frames, want)
    assert (status[0::4] == 0).all() and (status[1::4] == 1).all() and (frames[1::4] == sent[1::4]).all() and (status[2::4] == -1).any()


# ---- the second pass (tests/rs_cases.py below SHAPES): codes, depths and words the batches above never reach -------------------------

NEW_CASES = ([("case",) + s for s in rs_cases.GEOMETRY + rs_cases.DWORDS + rs_cases.TINY] + [("tiled",) + s for s in rs_cases.TILED]
             + [("sweep", name) for name in rs_cases.SWEEPS] + [("designed",) + d for d in rs_cases.DESIGNED]
             + [("miscorrecting", name) for name in rs_cases.MISCORRECTING] + [("many",)])
BUILDERS = dict(case=rs_cases.make_case, tiled=rs_cases.make_tiled, sweep=rs_cases.make_sweep, designed=rs_cases.make_designed,
                miscorrecting=rs_cases.make_miscorrecting, many=lambda: rs_cases.make_many()["base"])


def case_id(c):
    return "-".join("+".join(x) if isinstance(x, tuple) else str(x) for x in c)


@pytest.mark.parametrize("which", NEW_CASES, ids=case_id)
def test_package_rule_equals_the_reference_on_the_new_cases(which):
    case = BUILDERS[which[0]](*which[1:])
    rs_cases.check_seed(case)
    frames, status = rs.rs_decode_numpy(case["code"], case["got"], case["I"])
    assert status.dtype == np.int32 and status.shape == case["status"].shape
    assert np.array_equal(status, case["status"]), (status.reshape(-1).tolist(), case["status"].reshape(-1).tolist())
    assert np.array_equal(frames, case["want"])


def test_the_new_codes_cover_what_they_promise():
    codes = list(rs_cases.ALL_CODES.values())
    assert set(rs_cases.NEW_CODES).isdisjoint(rs_cases.CODES) and {s[0] for s in rs_cases.GEOMETRY} == set(rs_cases.NEW_CODES)
    assert {c.gfpoly for c in codes} == set(rs_cases.PRIMITIVE_POLYNOMIALS) and len(rs_cases.PRIMITIVE_POLYNOMIALS) == 16
    assert {0, 254} <= {c.fcr for c in codes}
    assert 254 in {c.prim for c in codes} and len({c.prim for c in codes} - {1, 7, 11, 254}) >= 2
    assert {2, 3, 4, 5, 6, 8, 9, 16, 17, 32, 33, 64} <= {c.nroots for c in codes}
    assert {2, 33, 64} <= {c.nroots for c in codes if c.n == c.nroots + 1}
    assert any(c.n == 252 and c.nroots >= 33 for c in codes)
    assert {1, 2, 3} <= {c.n % 4 for c in codes if c.nroots >= 33}
    for name, I, rows, max_frames in rs_cases.GEOMETRY:
        code = rs_cases.NEW_CODES[name]
        assert (rows, max_frames) == (3, 2) and I in ((5 if code.n <= 40 else 2), 1)
    assert {s[1] for s in rs_cases.TILED} == {9, 11, 16, 17, 64} and all(s[2] * s[3] > 1 for s in rs_cases.TILED)
    many = rs_cases.make_many()
    assert many["rows"] * many["max_frames"] > 65535 and many["got"].shape == (2, 35000, 3) and many["status"].shape == (2, 35000, 1)
    base = many["base"]
    assert len({w.tobytes() for w in base["got"][0]}) == 512 and set(base["counts"].reshape(-1).tolist()) == {0, 1, 2}
    assert set(base["status"].reshape(-1).tolist()) == {-1, 0, 1}
    flat = many["got"].reshape(-1, 3)
    assert np.array_equal(flat[512:1024], base["got"][0]) and np.array_equal(many["want"].reshape(-1, 3)[69632:], base["want"][0][:368])


@pytest.mark.parametrize("name", rs_cases.SWEEPS)
def test_every_sweep_holds_every_error_count_once(name):
    case = rs_cases.make_sweep(name)
    code, t = case["code"], case["code"].t
    assert case["got"].shape == (1, t + 3, code.n) and case["I"] == 1
    assert ((case["got"] != case["sent"]).sum(axis=2)[0] == np.arange(t + 3)).all()
    status = case["status"].reshape(-1).tolist()
    assert status[:t + 1] == list(range(t + 1))
    assert np.array_equal(case["want"][0, :t + 1], case["sent"][0, :t + 1])
    if t >= 8:                                                    # below that a word beyond t may rightly be moved to another codeword
        assert status[t + 1:] == [-1, -1]
    assert {name for name in rs_cases.SWEEPS if rs_cases.ALL_CODES[name].t >= 8} == {"ccsds223dual", "dvb", "nroots64", "n17", "n33"}


@pytest.mark.parametrize("name,kinds", rs_cases.DESIGNED, ids=[d[0] for d in rs_cases.DESIGNED])
def test_the_designed_words_are_what_they_are_called(name, kinds):
    case = rs_cases.make_designed(name, kinds)
    code = case["code"]
    M, rts = ref.mul_table(code.gfpoly), ref.roots(code.gfpoly, code.fcr, code.prim, code.nroots)
    assert len(case["kinds"]) == case["max_frames"] and {k[0] for k in case["kinds"]} == set(kinds)
    runs = {"lead": set(), "trail": set()}
    for what, sent, got, want, status in zip(case["kinds"], case["sent"][0], case["got"][0], case["want"][0], case["status"][0, :, 0]):
        S = ref.syndromes(M, rts, got)
        if what[0] == "fill":
            w, x = what[1:]
            assert status == -1 and np.array_equal(want, got) and int((got != sent).sum()) == x and w + x <= code.t and S.any()
            continue
        m = what[1]
        runs[what[0]].add(m)
        assert not ref.syndromes(M, rts, sent).any() and int((got != sent).sum()) == m + 1
        zero = (S[:m], S[m]) if what[0] == "lead" else (S[code.nroots - m:], S[code.nroots - m - 1])
        assert not zero[0].any() and zero[1] != 0
        if m + 1 <= code.t:
            assert status == m + 1 and np.array_equal(want, sent)
        else:
            assert status == -1 and np.array_equal(want, got)
    t = code.t
    for kind in set(kinds) - {"fill"}:
        assert runs[kind] == {m for m in (1, 2, t // 2, t - 1, t, t + 4) if 1 <= m < code.nroots} and max(runs[kind]) >= t
    if "fill" in kinds:
        fills = {k[1:] for k in case["kinds"] if k[0] == "fill"}
        w = min(t, code.pad)
        assert fills == {(1, 0), (1, t - 1), (w, 0), (w, t - w)}


@pytest.mark.parametrize("name", rs_cases.MISCORRECTING)
def test_the_miscorrecting_cases_hold_both_outcomes(name):
    case = rs_cases.make_miscorrecting(name)
    code = case["code"]
    assert 1 < code.t < 8 and case["got"].shape == (1, 300, code.n)
    errors = (case["got"] != case["sent"]).sum(axis=2)[0]
    assert np.array_equal(errors, code.t + 1 + np.arange(300) % 3)
    status = case["status"][0, :, 0]
    moved = (status >= 0) & (case["want"][0] != case["sent"][0]).any(axis=1)
    assert moved.sum() >= 20 and (status == -1).sum() >= 20 and np.array_equal(moved, status >= 0)
    print(name, "moved to another codeword:", int(moved.sum()), "of 300")


def build_tables_dump(tmp_path):
    """tests/cpp/rs_tables_dump.cpp as a program of its own, with the address and undefined-behaviour sanitizers where g++ links them"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rs_tables_dump")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(root, "tests", "cpp", "rs_tables_dump.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run(base, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def dump(lines=None):
        text = None if lines is None else "".join(" ".join(str(int(x)) for x in line) + "\n" for line in lines)
        q = subprocess.run([exe] + (["geometry"] if lines is None else []), input=text, capture_output=True, text=True, timeout=120)
        assert q.returncode == 0 and not q.stderr, q.stderr
        return q.stdout.splitlines()

    return dump


def test_host_tables_and_geometry_as_a_program_of_their_own(tmp_path):
    dump = build_tables_dump(tmp_path)
    # every odd polynomial with an x^8 term: accepted exactly where x is primitive, as RSCode says
    polys = list(range(0x101, 0x200, 2))
    answers = dump([(g, 1, 1, 2, 0, 0) for g in polys])
    assert len(answers) == 128
    accepted = []
    for g, line in zip(polys, answers):
        try:
            RSCode(g, 1, 1, 2)
            mine = True
        except ValueError:
            mine = False
        assert line.startswith("ok ") == mine == (g in rs_cases.PRIMITIVE_POLYNOMIALS), hex(g)
        if not mine:
            assert line == "invalid gfpoly is not primitive"
            continue
        accepted.append(g)
        blob = np.frombuffer(bytes.fromhex(line[3:]), dtype=np.uint8)
        assert blob.size == 1280
        M = ref.mul_table(g)
        powers = [1]
        for _ in range(254):
            powers.append(int(M[powers[-1], 2]))
        assert sorted(powers) == list(range(1, 256)) and int(M[powers[-1], 2]) == 1
        assert blob[:512].tolist() == [powers[i % 255] for i in range(512)]
        assert blob[512 + np.array(powers)].tolist() == list(range(255)) and blob[512] == 0
        assert np.array_equal(blob[768:1024], np.arange(256)) and np.array_equal(blob[1024:], np.arange(256))
    assert accepted == sorted(rs_cases.PRIMITIVE_POLYNOMIALS)
    # the dual basis
    plain, dual = dump([(0x187, 112, 11, 32, 0, 0), (0x187, 112, 11, 32, 0, 1)])
    plain, dual = (np.frombuffer(bytes.fromhex(x[3:]), dtype=np.uint8) for x in (plain, dual))
    to_dual, to_conv = ref.dual_tables(0x187)
    assert np.array_equal(dual[:768], plain[:768]) and np.array_equal(dual[768:1024], to_conv) and np.array_equal(dual[1024:], to_dual)
    # the parameter rule: what test_parameters_are_checked gives RSCode, and the edges beside it
    good = dict(gfpoly=0x187, fcr=112, prim=11, nroots=32, pad=0, dual_basis=0)
    bad = [dict(gfpoly=0x11B), dict(nroots=1), dict(nroots=65), dict(pad=230), dict(prim=3), dict(prim=0), dict(fcr=255), dict(gfpoly=0x87),
           dict(gfpoly=0x11D, dual_basis=1), dict(pad=223), dict(pad=255), dict(prim=255), dict(gfpoly=0x287), dict(dual_basis=2),
           dict(gfpoly=0x100), dict(gfpoly=0x11C)]
    fine = [dict(), dict(pad=222), dict(nroots=2, pad=252), dict(nroots=64, pad=190), dict(fcr=254, prim=254), dict(fcr=0, prim=1)]
    fields = ("gfpoly", "fcr", "prim", "nroots", "pad", "dual_basis")
    answers = dump([[{**good, **d}[f] for f in fields] for d in bad + fine])
    assert [a.split()[0] for a in answers] == ["invalid"] * len(bad) + ["ok"] * len(fine), answers
    for d in bad[:9]:
        with pytest.raises(ValueError):
            RSCode(**{**good, **d})
    # the syndrome geometry of every code there is
    rows = [tuple(int(x) for x in line.split()) for line in dump()]
    assert [r[:2] for r in rows] == [(nroots, n) for nroots in range(2, 65) for n in range(nroots + 1, 256)]
    for nroots, n, R2, G, seg, base in rows:
        assert R2 >= nroots and R2 < 2 * nroots and R2 & (R2 - 1) == 0 and R2 >= 2, (nroots, n)
        assert R2 * G == 64 and seg % 4 == 0 and seg > 0 and G * seg <= 256 and base == G * seg - n and base >= 0, (nroots, n)
