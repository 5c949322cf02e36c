"""ViterbiDecoder_HIP_Batch::dab_deinterleave and ::dab_descramble from C++ (tests/cpp/run_dab_hip.cpp): the program reads a case file this
test writes -- the shape, the inputs, and the images of every output buffer by the restatement of tests/dab_reference.py, fill and guard
included -- and prints PASS when the inputs and the outputs equal their images.  One small shape per call.  Built by
__graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from tests import dab_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_dab_hip")
GUARD = 16


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def _write(path, lines):
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(v)) for v in line) + "\n")


def write_deinterleave_case(path):
    """3 rows of 20 frames of 4-A n = 1 through the profile's map, per-row counts and fills, the output one element off a dword"""
    rng = np.random.default_rng(1)
    rows, mf, lead = 3, 20, 1
    mask = ref.mask_walk([(1, 3), (5, 2)])
    idx, n = ref.source_map(mask)
    assert n == 256 and len(idx) == 792
    frames = rng.integers(-32768, 32768, size=(rows, mf, n)).tolist()
    hists = rng.integers(-32768, 32768, size=(rows, ref.H, n)).tolist()
    counts, fills = [25, 7, 16], [15, 3, 99]
    out, n_out, hist_out, fill_out = ref.deinterleave_image(frames, counts, hists, fills, n, mf, idx, ref.POISON16)
    assert n_out == [20, 0, 16] and fill_out == [15, 10, 15]
    image = [ref.POISON16] * lead + out + [ref.POISON16] * GUARD
    flat = lambda x: np.asarray(x).reshape(-1).tolist()            # noqa: E731
    _write(path, [[0, rows, mf, n, len(idx), 1, 1, 1, lead, len(image)], counts, idx, fills, flat(hists), flat(frames), image, n_out,
                  flat(hist_out), fill_out])
    return out


def write_descramble_case(path, in_place):
    """2 rows of 5 frames of 771 bits at a stride of 99 bytes, per-row counts"""
    rng = np.random.default_rng(2)
    rows, mf, n_bits, stride = 2, 5, 771, 99
    frames = rng.integers(0, 256, size=(rows, mf, stride))
    counts = [5, 2]
    out = ref.descramble_image(frames.tolist(), counts, n_bits, mf, stride, before=frames.reshape(-1).tolist() if in_place else None)
    _write(path, [[1, rows, mf, n_bits, stride, 1, int(in_place)], counts, frames.reshape(-1).tolist(), out])
    return out


def test_run_dab_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deinterleave", "descramble", "descramble_in_place"])
def test_run_dab_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    want = write_deinterleave_case(path) if name == "deinterleave" else write_descramble_case(path, name.endswith("in_place"))
    assert any(v != 0 for v in want)
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches input=0, output=0, history=0, counts=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
