"""GSM channel decoding from C++ (tests/cpp/run_gsm_hip.cpp): ViterbiDecoder_HIP_Batch::gsm_deinterleave, ::gsm_fire and ::gsm_tchfs on one
small batch.  The program reads a case file this test writes -- random bursts with the outputs the numpy rule predicts in both modes,
the Fire frames of tests/gsm_cases.py with their statuses and LSB-first octets, decoded class I bytes and class II values with the speech
frames -- and prints PASS when every byte of every output buffer equals them.  Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import GSM_BLOCK, GSM_DIAGONAL, gsm_deinterleave_numpy, gsm_fire_numpy, gsm_tchfs_numpy
from tests import gsm_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_gsm_hip")
ROWS, M, FRAMES = 3, 5, 80


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path):
    rng = np.random.default_rng(17)
    bursts = rng.integers(-127, 128, size=(ROWS, 4 * M, 116)).astype(np.int16)
    lines = [[ROWS, M, FRAMES], bursts]
    for mode in (GSM_BLOCK, GSM_DIAGONAL):
        lines += list(gsm_deinterleave_numpy(bursts, mode)[:5])
    fire = cases.fire_frames()[0][:FRAMES]
    status, data = gsm_fire_numpy(fire, 12, lsb_first=True)
    decoded = rng.integers(0, 256, size=(FRAMES, 24), dtype=np.uint8)
    class2 = rng.integers(-3, 4, size=(FRAMES, 78)).astype(np.int16)
    speech, tstatus = gsm_tchfs_numpy(decoded, class2, cases.HIGH, cases.LOW)
    lines += [fire, status, data, decoded, class2, speech, tstatus]
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(v)) for v in np.asarray(line).reshape(-1)) + "\n")
    return status


def test_run_gsm_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_run_gsm_hip(tmp_path):
    _ensure_built()
    path = tmp_path / "case.txt"
    status = write_case(path)
    assert set(status[:, 0].tolist()) == set(range(-1, 13))
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches deinterleave=0, fire=0, tchfs=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
