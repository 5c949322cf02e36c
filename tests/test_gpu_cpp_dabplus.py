"""ViterbiDecoder_HIP_Batch::dabplus_sync and ::dabplus_au_table from C++ (tests/cpp/run_dabplus_hip.cpp): the program reads a case file
this test writes -- the shape, the inputs, and the images of every output buffer by the restatement of tests/dabplus_reference.py, the
0x5A fill where nothing is written included -- and prints PASS when the inputs and the outputs equal their images.  One small shape per
call.  Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from tests import dabplus_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_dabplus_hip")
FILL = 0x5A5A5A5A


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def _write(path, lines):
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(v)) for v in line) + "\n")


def flat(x):
    return np.asarray(x).reshape(-1).tolist()


def write_sync_case(path, accumulate):
    """3 rows of 12 frames of 48 bytes at a stride of 53, frame0 = 3, per-row counts (one above max_frames, one 0)"""
    rng = np.random.default_rng(1)
    rows, mf, fb, fs, frame0 = 3, 12, 48, 53, 3
    frames = rng.integers(0, 256, size=(rows, mf, fs))
    for r, phase in enumerate((4, 1, 2)):
        for f in range(mf):
            if (frame0 + f) % 5 == phase:
                c = ref.shift_register(frames[r, f].tolist(), 2, 9, 0x782F, 0)
                frames[r, f, 0], frames[r, f, 1] = c >> 8, c & 255
    counts = [12, 0, 99]
    before = (rng.integers(0, 5, size=(rows, 5)).tolist(), rng.integers(5, 9, size=(rows, 5)).tolist()) if accumulate else ([[0] * 5] * rows,) * 2
    hits, count, lock = ref.sync_image(frames.tolist(), counts, frame0, fb, *(before if accumulate else ()))
    _write(path, [[0, rows, mf, fb, fs, frame0, 1, int(accumulate)], counts, flat(frames), flat(before[0]), flat(before[1]), flat(hits),
                  flat(count), flat(lock)])
    return lock


def write_au_case(path, has_status):
    """2 rows of 3 superframes at s = 3 and a stride of 365 bytes, all four formats, a hostile header, per-row counts"""
    rng = np.random.default_rng(2)
    rows, mf, s, stride = 2, 3, 3, 365
    sfs = []
    for i in range(rows * mf):
        dac, sbr = [(0, 1), (1, 1), (0, 0), (1, 0)][i % 4]
        n, first = ref.FORMATS[(dac, sbr)]
        aus = [rng.integers(0, 256, size=L).tolist() for L in ref.split_lengths(110 * s - first, n, rng)]
        data = ref.build_data(aus, dac, sbr, s, i, starts=[0xFFF] * (n - 1) if i == 4 else None)
        sfs.append(data + rng.integers(0, 256, size=stride - 110 * s).tolist())
    sfs = [sfs[:mf], sfs[mf:]]
    counts = [3, 2]
    status = rng.integers(-1, 4, size=(rows, mf, s)).tolist()
    info, au = ref.au_image(sfs, counts, s, status if has_status else None, FILL)
    _write(path, [[1, rows, mf, s, stride, 1, int(has_status)], counts, flat(sfs), flat(status), info, au])
    return info


def test_run_dabplus_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sync", "sync_accumulate", "au", "au_status"])
def test_run_dabplus_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    want = write_sync_case(path, name.endswith("accumulate")) if name.startswith("sync") else write_au_case(path, name.endswith("status"))
    assert any(v != 0 for v in flat(want))
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches input=0, output=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
