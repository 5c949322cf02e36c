"""ViterbiDecoder_HIP_Batch::sync_search and ::sync_build from C++ (tests/cpp/run_sync_search_hip.cpp): the program reads a case
file this test writes -- the received buffer, the hypotheses and the counts and winner of the oracle-side composition
(tests/sync_reference.py) -- and prints PASS when the device's agree.  Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

from tests import sync_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_sync_search_hip")


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, c, errors, compared, best):
    source = [] if c["mask"] is None else ref.source_map(c["mask"])[0].tolist()
    kept = 0 if c["mask"] is None else ref.source_map(c["mask"])[1]
    rows = [[c["T"], c["W"], c["head"], c["tail"], c["received"].size, len(c["hypotheses"]), len(source), kept], source,
            [x for h in c["hypotheses"] for x in h], c["received"].tolist(), list(errors), list(compared), [best]]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(str(int(x)) for x in row) + "\n")


def test_run_sync_search_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["voyager", "voyager_3_4"])
def test_run_sync_search_hip(oracle, tmp_path, name):
    """Voyager soft16, 352 steps in 4 windows of 64: unpunctured under the four QPSK rotations, and the 3/4 mask under inversion"""
    _ensure_built()
    c = ref.make_case(name)
    errors, compared, best, _ = ref.case_reference(oracle, name)
    path = tmp_path / (name + ".txt")
    write_case(path, c, errors, compared, best)
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatching hypotheses=0," in p.stdout and "mismatching symbols of the winner's stream=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
