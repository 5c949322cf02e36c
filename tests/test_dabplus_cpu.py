"""DAB+ superframes without a GPU: dabplus.py against the independent restatement of tests/dabplus_reference.py, the transmit side
through the numpy rules and back for all four formats, and the kernels' device functions on the host under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from tests import dabplus_reference as ref
from viterbidecodercpp_amd import (DAB_CRC16, DABPLUS_RS_120_110, FIRECODE, crc_numpy, dabplus_au_table_numpy, dabplus_lock_numpy,
                                   dabplus_superframe_numpy, dabplus_sync_numpy, firecode_hit_numpy, frames_extract_numpy,
                                   rs_decode_numpy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [(0, 1), (1, 1), (0, 0), (1, 0)]


def test_the_codes():
    assert (FIRECODE.width, FIRECODE.poly, FIRECODE.init, FIRECODE.xorout) == (16, 0x782F, 0, 0)
    assert (DABPLUS_RS_120_110.n, DABPLUS_RS_120_110.k, DABPLUS_RS_120_110.nroots) == (120, 110, 10)
    msg = np.frombuffer(b"123456789", dtype=np.uint8)
    assert int(crc_numpy(FIRECODE, msg, 72)) == ref.shift_register(list(msg), 0, 9, 0x782F, 0)
    assert int(crc_numpy(DAB_CRC16, msg, 72)) == ref.au_crc(list(msg), 0, 9) == 0xD64E


def test_sync_against_the_restatement():
    rng = np.random.default_rng(1)
    for trial in range(6):
        rows, F, fb = int(rng.integers(1, 4)), int(rng.integers(0, 14)), int(rng.integers(11, 30))
        frames = rng.integers(0, 256, size=(rows, F, fb), dtype=np.uint8)
        for r in range(rows):
            for f in range(F):
                kind = rng.integers(0, 4)
                if kind == 0:
                    frames[r, f, :11] = 0
                elif kind < 3:
                    c = ref.shift_register(frames[r, f].tolist(), 2, 9, 0x782F, 0)
                    frames[r, f, 0], frames[r, f, 1] = c >> 8, c & 255
                    if kind == 2 and rng.integers(0, 2):
                        frames[r, f, rng.integers(0, 11)] ^= 1 << rng.integers(0, 8)
        counts = None if trial % 2 else [int(rng.integers(0, F + 3)) for _ in range(rows)]
        frame0 = int(rng.integers(0, 5))
        h0 = rng.integers(0, 9, size=(rows, 5))
        totals = None if trial % 3 else (h0, h0 + rng.integers(0, 9, size=(rows, 5)))
        hits, count, lock = dabplus_sync_numpy(frames, counts, frame0, totals=totals)
        want = ref.sync_image(frames.tolist(), counts, frame0, fb, *([] if totals is None else [t.tolist() for t in totals]))
        assert hits.tolist() == want[0] and count.tolist() == want[1] and lock.tolist() == want[2]
    assert not firecode_hit_numpy(np.zeros(24, dtype=np.uint8))
    # a tie goes to the lower phase; no hit at all is phase 0 with errors == compared
    assert dabplus_lock_numpy([[0, 2, 0, 2, 0]], [[3, 4, 3, 4, 3]], 24).tolist() == [[192, 0, 2, 4]]
    assert dabplus_lock_numpy([[0, 0, 0, 0, 0]], [[2, 2, 1, 1, 1]], 24).tolist() == [[0, 0, 2, 2]]
    with pytest.raises(ValueError):
        dabplus_sync_numpy(np.zeros((1, 2, 24), dtype=np.uint8), frame0=5)


@pytest.mark.parametrize("s", [1, 3, 24])
def test_au_table_against_the_restatement(s):
    rng = np.random.default_rng(10 + s)
    sfs, status = [], []
    for i in range(10):
        dac, sbr = FORMATS[i % 4]
        n, first = ref.FORMATS[(dac, sbr)]
        aus = [rng.integers(0, 256, size=L).tolist() for L in ref.split_lengths(110 * s - first, n, rng, fixed=(1,) if i == 4 else ())]
        hostile = {5: [0xFFF] * (n - 1), 6: [first + 2] * (n - 1), 7: [110 * s - 1 - k for k in range(n - 1)]}.get(i)
        data = ref.build_data(aus, dac, sbr, s, byte2_low=i, starts=hostile)
        if i == 8:
            data[110 * s - 1] ^= 0x10                              # a broken CRC in the last access unit alone, behind the Fire code's bytes
        if i == 9:
            data[1] ^= 1                                           # a broken Fire code
        sfs.append(data + rng.integers(0, 256, size=10 * s).tolist())
        status.append([-1 if (i == 3 and c == s - 1) else int(rng.integers(0, 6)) for c in range(s)])
    x = np.array(sfs, dtype=np.uint8).reshape(2, 5, 120 * s)
    for st in (None, np.array(status).reshape(2, 5, s)):
        info, au = dabplus_au_table_numpy(x, s, st)
        want = ref.au_image(x.tolist(), None, s, None if st is None else st.tolist(), 0)
        assert info.reshape(-1).tolist() == want[0] and au.reshape(-1).tolist() == want[1]
    assert (info.reshape(-1)[[5, 6, 7]] & 2 == 0).all() and info.reshape(-1)[9] & 1 == 0 and info.reshape(-1)[3] & 4
    syn = au.reshape(10, 6, 3)[8, :, 2]
    assert syn[:2].tolist() == [0, 0x10]                           # format (0, 1): two access units


@pytest.mark.parametrize("dac,sbr", FORMATS)
def test_transmit_side_round_trip(dac, sbr):
    """superframe -> dabplus_sync_numpy -> frames_extract_numpy -> rs_decode_numpy (5 byte errors in every codeword) ->
    dabplus_au_table_numpy returns the access units sent"""
    rng = np.random.default_rng(4 + 2 * dac + sbr)
    s = 3
    n, first = ref.FORMATS[(dac, sbr)]
    sent, frames = [], [rng.integers(0, 256, size=(2, 24 * s), dtype=np.uint8)]      # two frames of fill in front
    for _ in range(2):
        aus = [rng.integers(0, 256, size=L, dtype=np.uint8) for L in ref.split_lengths(110 * s - first, n, rng)]
        sent.append(aus)
        frames.append(dabplus_superframe_numpy(aus, dac, sbr, s, byte2_low=9))
    frames = np.concatenate(frames)
    assert frames.shape == (12, 24 * s)
    assert frames[2:7].reshape(-1)[:110 * s].tolist() == ref.build_data([a.tolist() for a in sent[0]], dac, sbr, s, 9)
    hits, count, lock = dabplus_sync_numpy(frames, frame0=4)
    assert lock.tolist() == [[1 * 8 * 24 * s, 0, 0, 2]]           # frame 2 is of phase (4 + 2) mod 5
    got, _, carry, rem = frames_extract_numpy(frames.reshape(-1), frames.size * 8, 960 * s, 4 * 192 * s, lock[0])
    assert got.shape == (2, 120 * s) and rem == 0
    for c in range(s):
        for f in range(2):
            got[f, c + s * rng.choice(120, size=5, replace=False)] ^= rng.integers(1, 256, size=5).astype(np.uint8)
    fixed, status = rs_decode_numpy(DABPLUS_RS_120_110, got, s)
    assert (status == 5).all()
    info, au = dabplus_au_table_numpy(fixed, s, status)
    assert info.tolist() == [3 | n << 4 | (dac << 6 | sbr << 5 | 9) << 8] * 2
    for f in range(2):
        for k in range(6):
            start, nb, syn = au[f, k]
            if k < n:
                assert syn == 0 and fixed[f, start:start + nb].tolist() == sent[f][k].tolist()
            else:
                assert (start, nb, syn) == ref.EMPTY
    with pytest.raises(ValueError):
        dabplus_superframe_numpy(sent[0][:-1], dac, sbr, s)


def test_the_kernel_source_on_the_host_under_the_sanitizers(tmp_path):
    """tests/cpp/dabplus_host_check.cpp: the kernels' device functions compiled by g++ with the HIP built-ins stubbed, as a program of its
    own -- with the address and undefined-behaviour sanitizers where g++ links them --, run as a child process: random shapes of both
    kernels whose inputs end their heap blocks, hostile headers, against a bit-by-bit restatement.  In front of the shapes the
    program walks both argument rules: an accepted call, every INVALID_ARG case of tests/test_gpu_dabplus.py, the zero-work cases.  Only
    where the linker reports that it cannot find a sanitizer's runtime is the program built without them, and the test prints which build ran"""
    exe = str(tmp_path / "dabplus_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "dabplus_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("dabplus_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe, "300", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 300 shapes"), q.stdout
