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
    code = CODES[name]
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
