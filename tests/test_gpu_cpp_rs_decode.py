"""ViterbiDecoder_HIP_Batch::rs_create / rs_decode from C++ (tests/cpp/run_rs_decode_hip.cpp): the program reads a case file this test
writes -- the code, the frames, the frame counts and the images of the frame and status buffers by the rule of tests/rs_reference.py --
and prints PASS when the call in place and the call out of place both equal the images byte for byte.
Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from tests import rs_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_rs_decode_hip")
POISON32 = -1515870811                                            # 0xA5A5A5A5 as int32

# shape of tests/rs_cases.py, guard bytes behind every frame, frame counts or None
CASES = {
    "ccsds": (("ccsds223dual", 5, 2, 5), 3, [4, 9]),
    "dvb": (("dvb", 1, 2, 5), 0, None),
    "short": (("short", 8, 1, 1), 5, None),
    "deep": (("dvb", 11, 2, 5), 3, [4, 9]),                       # two tiles of codewords in every frame
}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, shape, extra, counts):
    case = rs_cases.make_case(*shape)
    code, I, rows, mf = case["code"], case["I"], case["rows"], case["max_frames"]
    nI = code.n * I
    src = np.full((rows, mf, nI + extra), 0x5A, dtype=np.uint8)
    src[..., :nI] = case["got"]
    image, status = src.copy(), np.full((rows, mf, I), POISON32, dtype=np.int64)
    for r in range(rows):
        live = mf if counts is None else min(counts[r], mf)
        image[r, :live, :nI] = case["want"][r, :live]
        status[r, :live] = case["status"][r, :live]
    lines = [[code.gfpoly, code.fcr, code.prim, code.nroots, code.pad, int(code.dual_basis), I, rows, mf, nI + extra, int(counts is not None)],
             counts or [], src.reshape(-1).tolist(), image.reshape(-1).tolist(), status.reshape(-1).tolist()]
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(x)) for x in line) + "\n")
    return status


def test_run_rs_decode_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_rs_decode_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    status = write_case(path, *CASES[name])
    assert (status > 0).any() and (status == -1).any()
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches in place=0, out of place=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
