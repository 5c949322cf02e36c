"""The front of the DVB-T route from C++ (tests/cpp/run_dvbt_hip.cpp): ViterbiDecoder_HIP_Batch::dvbt_deinterleave against a host loop of
the rule, one mode per constellation, rows at strides of their own, the parity counters on the device.  The program needs no case file
and prints PASS when every byte of every output buffer and every counter is as the rule says.  Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_dvbt_hip")


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def test_run_dvbt_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_run_dvbt_hip():
    _ensure_built()
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("mismatches 0, counters ok") == 3
    assert p.stdout.strip().endswith("PASS"), p.stdout
