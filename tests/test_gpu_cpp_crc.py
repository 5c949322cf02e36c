"""ViterbiDecoder_HIP_Batch::crc_check from C++ (tests/cpp/run_crc_hip.cpp): the program reads a case file this test writes -- the code,
the shape, the frames at an odd base address and stride, the counts, and the images of both outputs by the long division of
tests/crc_reference.py -- and prints PASS when the input and both outputs equal their images, written or not.
Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

from tests import crc_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_crc_hip")

# width, n_bits, first_bit, rows, max_frames, field, counts, want_crc
CASES = {
    "lte": (16, 43, 0, 1, 300, True, None, True),                  # one lane a frame, a ragged last wave
    "ccsds": (16, 8904, 0, 3, 7, True, (7, 0, 3), True),           # 64 lanes a frame, counts
    "crc24_unaligned": (24, 1032, 13, 2, 5, True, (9, 2), False),  # the syndrome alone
    "crc32_alone": (32, 264, 7, 3, 2, False, None, True),          # the CRC alone: a frame ends with its data
    "one_bit": (1, 65, 1, 1, 1, True, None, True),
}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, width, n_bits, first_bit, rows, mf, field, counts, want_crc):
    case = ref.make_case(width, n_bits, first_bit, rows, mf, field, lead=3, slack=2, counts=counts)
    code, stride = case["code"], case["stride"]
    padded = list(case["buffer"]) + [ref.GUARD] * (case["lead"] + rows * mf * stride - case["buffer"].size)     # the program reads whole strides
    crc = case["crc"] if want_crc else case["crc"] * 0 + ref.POISON32
    lines = [[code.width, code.poly, code.init, code.xorout, rows, mf, stride, case["lead"], first_bit, n_bits, int(counts is not None),
              int(want_crc), int(field)], counts or [0] * rows, padded, crc.reshape(-1), case["syndrome"].reshape(-1)]
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(v)) for v in line) + "\n")
    return case


def test_run_crc_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_crc_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    case = write_case(path, *CASES[name])
    assert (case["crc"] != ref.POISON32).any()
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches input=0, crc=0, syndrome=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
