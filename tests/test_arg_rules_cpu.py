"""viterbidecodercpp_amd/csrc/arg_rules.hpp, the vocabulary every argument rule of the C ABI is worded in (overlap, extent, misaligned),
run on the host as a program of its own (tests/cpp/arg_rules_host_check.cpp).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_helpers_on_the_host(tmp_path):
    """tests/cpp/arg_rules_host_check.cpp: plain C++ compiled by g++, as a program of its own with the address and undefined-behaviour
    sanitizers, run as a child process.  Only where the linker reports that it cannot find a sanitizer's runtime is the program built
    without them; any other failure of the sanitizer build fails the test, and the test prints which build ran"""
    exe = str(tmp_path / "arg_rules_host_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "arg_rules_host_check.cpp")]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    sanitized = p.returncode == 0
    if not sanitized:
        assert any("cannot find" in line and "san" in line for line in p.stderr.splitlines()), p.stderr
        p = subprocess.run(base, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    print("arg_rules_host_check built", "with the address and undefined-behaviour sanitizers" if sanitized else "WITHOUT sanitizers: no runtime to link")
    q = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert q.returncode == 0 and not q.stderr, q.stdout + q.stderr
    assert "the sum form answers 0 for a range inside it, the difference form 1" in q.stdout, q.stdout
    assert q.stdout.splitlines()[-1] == "ok: overlap, extent, misaligned", q.stdout
