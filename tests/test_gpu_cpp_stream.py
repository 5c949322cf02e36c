"""ViterbiDecoder_HIP_Batch::decode_stream from C++ (tests/cpp/run_continuous_hip.cpp): one long stream in chained segments against
the overlapped-window rule restated on the oracle's update / chainback.  Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_continuous_hip")


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def test_run_continuous_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_run_continuous_hip():
    """Voyager soft16 at the defaults (W = 1024, 48 steps each side) and K = 5 soft8 at W = 67, head 9, tail 13: every segment's
    bytes, bit count and pad bits"""
    _ensure_built()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("mismatching segments=0") == 2 and p.stdout.strip().endswith("PASS"), p.stdout
