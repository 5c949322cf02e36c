"""Tail-biting decoding without a GPU: the C ABI and C++ surfaces exist, the rule restated on the CPU checker decodes tail-biting
codewords of every stock code, and its default extension (8*(K-1) steps each side) is as good as exact maximum likelihood."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from viterbidecodercpp_amd import COMMON_CODES, _lib, get_decoding_config, synth

from tests.helpers import DECODE_TYPES, oracle_cfg
from tests.tb_reference import ml_tail_biting, tb_frames, tb_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB_SYMBOLS = ["vit_hip_tail_biting_workspace_bytes", "vit_hip_decode_tail_biting_batch"]


def test_tail_biting_exports():
    lib = _lib.load()
    for name in TB_SYMBOLS:
        assert name in _lib.EXPORTS
        getattr(lib, name)


def test_tail_biting_cpp_surface(tmp_path):
    src = tmp_path / "tb.cpp"
    src.write_text(
        '#include "viterbi_hip/viterbi_decoder_hip_batch.h"\n'
        "void f(ViterbiDecoder_HIP_Batch<7, 3, uint16_t, int16_t>& d, const int16_t* sym, void* ws, uint8_t* out,\n"
        "       uint32_t* ends, uint8_t* ok) {\n"
        "    const size_t n = d.tail_biting_workspace_bytes(100, 40);\n"
        "    d.decode_tail_biting(sym, 100, 40, ws, n, out);\n"
        "    d.decode_tail_biting(sym, 100, 40, ws, d.tail_biting_workspace_bytes(100, 40, 13, 19), out, ends, ok, 13, 19, nullptr);\n"
        "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_tail_biting_encoder_definition():
    """x[L-K+1:] ++ x through the zero-start encoder, outputs of steps K-1 .. K-2+L"""
    code = COMMON_CODES[3]
    rng = np.random.default_rng(5)
    L = 41
    x = rng.integers(0, 2, size=(2, L), dtype=np.uint8)
    got = synth.encode_tail_biting_numpy(code.K, code.R, code.G, x)
    for f in range(2):
        y = np.concatenate([x[f, L - code.K + 1:], x[f]])
        for t in range(L):
            for i in range(code.R):
                want = 0
                for k in range(code.K):
                    if (code.G[i] >> k) & 1:
                        want ^= int(y[t + code.K - 1 - k])
                assert got[f, t, i] == want


# Every stock code x decode type but Cassini SOFT8: with EVERY state a start state its 8-bit metrics (max_error 36 per step, K = 15)
# wrap before the survivors merge, and the rule -- which keeps the reference's wrapping error_t -- misdecodes some noise-free frames
# (the terminated decode starts from one state and does not).  The GPU still matches tb_reference bit for bit there.
NOISE_FREE_EXACT = [(c, t) for c in COMMON_CODES for t in DECODE_TYPES if not (c.K == 15 and t == "SOFT8")]


@pytest.mark.parametrize("code,decode_type", NOISE_FREE_EXACT, ids=lambda x: getattr(x, "name", x))
def test_reference_restatement_noise_free(oracle, code, decode_type):
    pc = get_decoding_config(decode_type, code.R)
    ocfg = oracle_cfg(decode_type, code.R)
    F = 2 if code.K >= 15 else 6
    for L in (code.K, 40, 41, 57):
        bits, sym = tb_frames(code, pc, F, L, None, seed=L + 100 * code.K + code.R)
        out, ends, ok = tb_reference(oracle, code, ocfg, sym, L)
        assert np.array_equal(np.unpackbits(out, axis=1)[:, :L], bits), (code.name, L)
        assert np.all(np.unpackbits(out, axis=1)[:, L:] == 0)
        assert np.all(ok == 1)
        # a noise-free path ends in the frame's own state: the last K-1 bits of the extension are those before the tail
        assert np.all(ends < (1 << (code.K - 1)))


# LTE K = 7, R = 1/3 SOFT16, L = 40 (the PDCCH size class): about 10 % and 1 % frame error rate
@pytest.mark.parametrize("ebn0", [1.0, 2.25])
def test_default_extension_is_near_maximum_likelihood(oracle, ebn0):
    code = COMMON_CODES[3]
    assert (code.K, code.R) == (7, 3)
    pc = get_decoding_config("SOFT16", code.R)
    ocfg = pyoracle.stock_config(pyoracle.SOFT16, code.R)
    F, L = 600, 40
    bits, sym = tb_frames(code, pc, F, L, ebn0, seed=int(ebn0 * 100) + 7)
    ml = ml_tail_biting(code, sym, L)
    out, _, _ = tb_reference(oracle, code, ocfg, sym, L)
    got = np.unpackbits(out, axis=1)[:, :L]
    ml_errors = int((ml != bits).any(axis=1).sum())
    tb_errors = int((got != bits).any(axis=1).sum())
    assert ml_errors > 0, "the operating point must produce frame errors"
    assert tb_errors <= 1.1 * ml_errors + 3, (tb_errors, ml_errors)
