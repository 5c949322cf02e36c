"""ViterbiDecoder_HIP_Batch::deinterleave / dvb_derandomize from C++ (tests/cpp/run_dvb_hip.cpp): the program reads a case file this
test writes -- the shape, the packets, counts, fills, phases and history, and the images of every output buffer by the numpy rules of
viterbidecodercpp_amd.dvb -- and prints PASS when every buffer equals its image, written or not.
Built by __graft_entry__.build()."""
import os
import subprocess

import numpy as np
import pytest

from viterbidecodercpp_amd import conv_deinterleave_numpy, conv_interleave_numpy, dvb, dvb_derandomize_numpy, dvb_randomize_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "run_dvb_hip")
POISON, POISON32 = 0xA5, 0xA5A5A5A5

# (branches, cell, packet_bytes), rows, max_frames, guard bytes, counts, fills or None (no history), phases or None (no derandomising)
CASES = {
    "dvb": ((12, 17, 204), 2, 30, 0, [30, 21], [11, 4], [8, 3]),
    "guarded": ((12, 17, 204), 3, 14, 3, [14, 0, 40], None, [0xFFFFFFFF, 2, 8]),
    "small": ((4, 3, 8), 3, 14, 1, [0, 5, 14], [0, 5, 9], None),
    "odd": ((3, 5, 9), 2, 9, 0, [9, 7], [4, 1], None),
}


def _ensure_built():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()


def write_case(path, shape, rows, mf, guard, counts, fills, phases):
    B, M, n = shape
    H = dvb.history_packets(B, M, n)
    rng = np.random.default_rng([B, M, n, rows, mf])
    if n == 204:                                                   # real DVB-S packets, so that the phase vote has sync bytes to read
        ts = rng.integers(0, 256, size=(rows, mf + H, 188), dtype=np.uint8)
        ts[..., 0] = 0x47
        sent = np.array([conv_interleave_numpy(np.pad(dvb_randomize_numpy(t, 5), ((0, 0), (0, 16))), B, M) for t in ts])
        hist, x = sent[:, :H], sent[:, H:]
    else:
        hist, x = (rng.integers(0, 256, size=(rows, k, n), dtype=np.uint8) for k in (H, mf))
    src = np.full((rows, mf, n + guard), 0x5A, dtype=np.uint8)
    src[..., :n] = x
    out = np.full((rows, mf, n + guard), POISON, dtype=np.uint8)
    hist_out = np.full((rows, H, n), POISON, dtype=np.uint8)
    n_out, fill_out = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    packets = np.full((rows, mf, 188), POISON, dtype=np.uint8)
    phase_out, sync_errors = np.zeros(rows, dtype=np.int64), np.full((rows, mf), POISON32, dtype=np.int64)
    for r in range(rows):
        got, n_out[r], new, fill_out[r] = conv_deinterleave_numpy(x[r], B, M, None if fills is None else hist[r], 0 if fills is None else fills[r],
                                                                  counts[r])
        out[r, :n_out[r], :n] = got
        hist_out[r, H - fill_out[r]:] = new[H - fill_out[r]:]
        if phases is not None:
            ts_out, errors, phase_out[r] = dvb_derandomize_numpy(got, phases[r])
            packets[r, :len(ts_out)] = ts_out
            sync_errors[r, :len(errors)] = errors
    lines = [[B, M, n, rows, mf, n + guard, int(fills is not None), int(phases is not None)], counts, fills or [0] * rows, phases or [0] * rows,
             src.reshape(-1), hist.reshape(-1) if fills is not None else [], out.reshape(-1), n_out, hist_out.reshape(-1), fill_out]
    if phases is not None:
        lines += [packets.reshape(-1), phase_out, sync_errors.reshape(-1)]
    with open(path, "w") as f:
        for line in lines:
            f.write(" ".join(str(int(v)) for v in line) + "\n")
    return n_out, packets


def test_run_dvb_hip_builds():
    _ensure_built()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_dvb_hip(tmp_path, name):
    _ensure_built()
    path = tmp_path / (name + ".txt")
    n_out, packets = write_case(path, *CASES[name])
    assert n_out.sum() > 0 and (n_out < CASES[name][2]).any()
    if name == "dvb":                                              # full history: the transport packets come back, sync byte upright
        assert (packets[0, :n_out[0], 0] == 0x47).all() and n_out[0] == 30
    p = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches input=0, deinterleave=0, derandomize=0" in p.stdout
    assert p.stdout.strip().endswith("PASS"), p.stdout
