"""ViterbiDecoder_HIP_Batch::lte_rate_dematch from C++ (tests/cpp/run_lte_dematch_hip.cpp): the program reads a case file this test
writes -- the shape, the soft bits, offsets, counts, the mask, and the image of the output buffer by the scalar loop of
tests/lte_reference.py, fill and guard included -- and prints PASS when the input and the output equal their images.
Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from tests import lte_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_lte_dematch_hip")

# frames, D, E_max, stride (None: offsets and counts), mask ("none", "shared", "region"), shift, clamp, lead
CASES = {
    "pbch": (5, 40, 1920, 1920, "shared", 4, (-127, 127), 0),
    "pdcch_region": (15, 43, 576, None, "region", 0, (-127, 127), 1),
    "punctured_stride": (300, 43, 72, 75, "none", 1, (-32768, 32767), 1),
    "ragged": (3, 65, 395, 400, "shared", 0, (-1000, 900), 0),
}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, frames, D, E_max, stride, mask, shift, clamp, lead):
    rng = np.random.default_rng(frames * 1000 + D)
    if stride is None:
        n = 2001
        offsets = rng.integers(0, n + 3, size=frames).tolist()
        counts = rng.integers(0, E_max + 2, size=frames).tolist()
        offsets[:3], counts[:3] = [0, n - 1, 1], [E_max, E_max, 72]
    else:
        n, offsets, counts = (frames - 1) * stride + E_max, None, None
    received = rng.integers(-32768, 32768, size=n).astype(np.int16) if frames < 100 else rng.integers(-9, 10, size=n).astype(np.int16)
    period = {"none": 0, "shared": stride, "region": 0}[mask]
    bits = None if mask == "none" else rng.integers(0, 2, size=period or n).tolist()
    want = ref.dematch(received.tolist(), frames, D, E_max, stride=stride or 0, offsets=offsets, counts=counts, mask_bits=bits, period=period,
                       shift=shift, lo=clamp[0], hi=clamp[1])
    image = [ref.POISON16] * lead + want + [ref.POISON16] * ref.GUARD
    packed = [] if bits is None else ref.pack_bits(bits).tolist()
    lines = [[frames, D, E_max, n, stride or 0, int(offsets is not None), int(counts is not None), len(packed), period, shift, clamp[0], clamp[1],
              lead, len(image)], offsets or [0] * frames, counts or [0] * frames, packed, received.tolist(), image]
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(v)) for v in line) + "\n")
    return want


def test_run_lte_dematch_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_lte_dematch_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    want = write_case(path, *CASES[name])
    assert any(v != 0 for v in want)
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches input=0, output=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
