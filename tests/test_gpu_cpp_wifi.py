"""The 802.11a/g receive chain from C++ (tests/cpp/run_wifi_hip.cpp): ViterbiDecoder_HIP_Batch::wifi_deinterleave, ::decode,
::wifi_signal_parse and ::wifi_descramble, the per-frame arguments of the DATA stages pointing into the SIGNAL structs on the device.
The program reads a case file this test writes -- the soft bits of noisy PPDUs of mixed rate and length and the arrays of the CPU
composition (tests/wifi_cases.py), the PSDU image with its fill -- and prints PASS when all three outputs equal them.
Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from tests import wifi_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_wifi_hip")

# frames, max_sym, noise
CASES = {"mixed": (24, 4, 0.2), "one_frame": (1, 2, 0.0), "clean": (40, 3, 0.0)}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, frames, max_sym, sigma):
    specs = [(f % 8, 1 + (41 * f) % cases.largest_length(f % 8, max_sym), 1 + (31 * f) % 127) for f in range(frames)]
    signal_soft, data_soft, psdus = cases.make_ppdus(specs, max_sym, seed=frames, sigma=sigma)
    image, status, signal = cases.cpu_chain(signal_soft, data_soft, max_sym)
    assert (signal[:, 4] == 1).all() and status[:, 0].tolist() == [s[1] for s in specs]          # the CPU side recovers every frame
    assert all(status[f, 3] == 0 for f, s in enumerate(specs) if s[1] >= 4)
    with open(path, "w") as f:
        for line in ([frames, max_sym, image.shape[1]], signal_soft.reshape(-1), data_soft.reshape(-1), signal.reshape(-1), status.reshape(-1),
                     image.reshape(-1)):
            f.write(" ".join(str(int(v)) for v in line) + "\n")
    return image


def test_run_wifi_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_wifi_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    image = write_case(path, *CASES[name])
    assert (image != cases.FILL).any() and (image[:, -1] == cases.FILL).any()
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches signal=0, status=0, psdu=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
