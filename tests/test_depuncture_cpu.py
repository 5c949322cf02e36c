"""Depuncturing on the host: the kernel's own source run on the host under the address and undefined-behaviour sanitizers with map
values from all of int32 (tests/cpp/depuncture_host_check.cpp), and the ABI's answer to a NULL handle.  No GPU."""
import ctypes as C
import os
import subprocess

from viterbidecodercpp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_source_on_the_host_under_sanitizers(tmp_path):
    """tests/cpp/depuncture_host_check.cpp: depuncture_kernel compiled by g++ with the HIP built-ins stubbed, one thread per block, as a
    program of its own -- with the address and undefined-behaviour sanitizers where g++ links them: 400 random shapes of both symbol
    widths, the input, the map and the output in heap blocks of exactly their size, the map drawn from all of int32, every output
    against the rule in a plain loop.  An entry at or above punctured_per_frame that the kernel followed would read outside a block"""
    exe = str(tmp_path / "depuncture_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "depuncture_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if p.returncode != 0:
        p = subprocess.run(base, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    q = subprocess.run([exe, "400", "1"], capture_output=True, text=True, timeout=300)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert q.stdout.startswith("ok: 400 shapes of both widths"), q.stdout


def test_null_handle_is_rejected_without_a_device():
    lib = _lib.load()
    out = (C.c_int16 * 8)(*([0x5A5A] * 8))
    src = (C.c_int16 * 8)()
    idx = (C.c_int32 * 8)()
    rc = lib.vit_hip_depuncture_batch(None, C.cast(src, C.c_void_p), 8, C.cast(idx, C.c_void_p), 8, 1, C.cast(out, C.c_void_p), None)
    assert rc == _lib.ERR_INVALID_ARG and b"NULL handle" in lib.vit_hip_last_error()
    assert list(out) == [0x5A5A] * 8
