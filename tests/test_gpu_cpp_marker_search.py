"""ViterbiDecoder_HIP_Batch::marker_search from C++ (tests/cpp/run_marker_search_hip.cpp): the program reads a case file this test
writes -- rows of bytes, the marker, the history and the per-phase totals and locks of the numpy rule (tests/marker_reference.py) --
and prints PASS when one call, and two accumulating calls over the halves, agree.  Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

from tests import marker_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_marker_search_hip")

CASES = {
    "ccsds": dict(rows=3, n_bits=4099, m=32, P=1024, marker=0x1ACFFC1D, hb=31, phase0=1000, stride_extra=5, plant=(300, 1)),
    "dvb": dict(rows=2, n_bits=20_000, m=8, P=1632, marker=0x47, hb=0, phase0=0, stride_extra=0, plant=(1631, 0)),
    "m64": dict(rows=1, n_bits=1000, m=64, P=13, hb=63, phase0=12, stride_extra=1),
}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, c, distance, count, lock):
    history = [0] * c["rows"] if c["history"] is None else [int(x) for x in c["history"]]
    rows = [[c["rows"], c["n_bits"], c["stride"], c["marker"] >> 32, c["marker"] & 0xFFFFFFFF, c["m"], c["P"], c["phase0"], c["hb"]],
            [x for w in history for x in (w >> 32, w & 0xFFFFFFFF)], c["bytes"].reshape(-1).tolist(), distance.reshape(-1).tolist(),
            count.reshape(-1).tolist(), lock.reshape(-1).tolist()]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(str(int(x)) for x in row) + "\n")


def test_run_marker_search_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_marker_search_hip(tmp_path, name):
    _ensure_built()
    c = mr.make_case(len(name), **CASES[name])
    path = tmp_path / (name + ".txt")
    write_case(path, c, *mr.case_reference(c))
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches of one call=0, of two accumulating calls=0" in p.stdout and "too short to cut" not in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
