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
