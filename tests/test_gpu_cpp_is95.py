"""The IS-95A forward traffic channel from C++ (tests/cpp/run_is95_hip.cpp): ViterbiDecoder_HIP_Batch::is95_deinterleave,
::is95_channel_errors and ::is95_rate_decide on one small batch of mixed rates.  The program reads a case file this test writes -- noisy frames with a mask each,
the four outputs the numpy rule predicts, the decodes, counts and syndromes of the CPU composition (tests/is95_cases.py) and the decision
and info bytes the numpy rule makes of them -- and prints PASS when every byte of every output buffer equals them.
Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import is95_rate_decide_numpy
from tests import is95_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_is95_hip")
FRAMES = 12


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path):
    symbols, scramble, rates, info = cases.make_frames(cases.STOCK, frames=FRAMES, seed=12, snr_db=cases.NOISY_SNR_DB)
    sym, decoded, errors, compared, syndrome = cases.cpu_stages(cases.STOCK, symbols, scramble)
    counted = [np.array(e) for e in errors] + [np.array(c) for c in compared]
    syndrome[0][5] ^= 0x800                                           # one frame whose check fails, one whose counts are too bad
    errors[rates[7]][7] = compared[rates[7]][7]
    num, den = cases.MAX_SER
    decision, got = is95_rate_decide_numpy(decoded, errors, compared, syndrome, num, den)
    good = [f for f in range(FRAMES) if f not in (5, 7) or (f == 5 and rates[5] != 0)]
    assert decision[good, 0].tolist() == rates[good].tolist() and np.array_equal(got[good], info[good]) and decision[7, 0] != rates[7]
    with open(path, "w") as f:
        for line in ([FRAMES], symbols, scramble, *sym, *decoded, *errors, *compared, *syndrome, num, [den], decision, got, *counted):
            f.write(" ".join(str(int(v)) for v in np.asarray(line).reshape(-1)) + "\n")
    return decision


def test_run_is95_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_run_is95_hip(tmp_path):
    _ensure_built()
    path = tmp_path / "mixed.txt"
    decision = write_case(path)
    assert len(set(decision[:, 0].tolist())) >= 4
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches out=0, counts=0, decision=0, info=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
