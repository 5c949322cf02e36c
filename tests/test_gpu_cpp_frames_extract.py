"""ViterbiDecoder_HIP_Batch::frames_extract from C++ (tests/cpp/run_frames_extract_hip.cpp): the program reads a case file this test
writes -- rows of bytes, carries, locks, the pad and the images of every output buffer by the rule of tests/frames_reference.py -- and
prints PASS when one call equals the images byte for byte and two calls over the halves, the carry handed on, give the same frames.
Built by __graft_entry__.build()."""
import os
import subprocess

import pytest

from tests import frames_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_frames_extract_hip")

CASES = {
    "ccsds": dict(rows=3, n_bits=5 * 1024 + 77, P=1024, phase0=1000, c=[0, 9, 1023], skip=None, inverted=2, d=32, m=32, marker=0x1ACFFC1D,
                  pad=True, stride_extra=5, carry_extra=3),
    "dvb": dict(rows=2, n_bits=20_000, P=1632, phase0=0, c=[1631, 8], skip=1, inverted=1, d=8, m=8, marker=0x47, stride_extra=0),
    "odd": dict(rows=1, n_bits=1000, P=67, phase0=66, c=7, skip=0, inverted=0, d=5, m=64, pad=True, stride_extra=1, max_extra=2),
}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, c, images):
    frames, n, errors, carry, bits = images
    rows = [[c["rows"], c["n_bits"], c["stride"], c["P"], c["phase0"], c["marker"] >> 32, c["marker"] & 0xFFFFFFFF, c["m"], c["d"],
             int(c["pad"] is not None), c["max_frames"], c["cstride"]],
            c["lock"].reshape(-1).tolist(), c["carry_bits"].tolist(), c["carry"].reshape(-1).tolist(), c["bytes"].reshape(-1).tolist(),
            [] if c["pad"] is None else c["pad"].tolist(), n.tolist(), bits.tolist(), frames.tolist(), errors.tolist(), carry.tolist()]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(str(int(x)) for x in row) + "\n")


def test_run_frames_extract_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_frames_extract_hip(tmp_path, name):
    _ensure_built()
    c = fr.make_case(len(name), **CASES[name])
    assert c["fstride"] == c["qb"]
    path = tmp_path / (name + ".txt")
    write_case(path, c, fr.images(c, fr.case_reference(c)))
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches of one call=0, of two calls=0" in p.stdout and "too short to cut" not in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
