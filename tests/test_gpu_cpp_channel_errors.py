"""ViterbiDecoder_HIP_Batch::encode and ::channel_errors from C++ (tests/cpp/run_channel_errors_hip.cpp): synth -> decode ->
channel_errors against the counting rule applied on the host to the oracle's encoder.  Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_channel_errors_hip")


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def test_run_channel_errors_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_run_channel_errors_hip():
    """Voyager soft16, 130 frames of 1024 bits at 2 dB, and LTE hard8, 64 frames of 41 bits with inverted and erased symbols"""
    _ensure_built()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("mismatching frames=0, mismatching encoded symbols=0") == 2 and p.stdout.strip().endswith("PASS"), p.stdout
