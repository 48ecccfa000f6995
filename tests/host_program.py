"""Stand-alone host programs of the tests (a tests/*_main.cpp with its own main beside the product's GPU-free sources): the one compiler
search, the one flag list with AddressSanitizer + UBSan, the one environment they run in and the one pair of conditions on what a
sanitizer would have written.  A program is run as a child process; nothing here is loaded into Python.  No tests in here."""
import os
import shutil
import subprocess

import pytest

from tests.cli_run import ROOT

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def build(sources, out, sanitize=True, libs=(), skip_without_compiler=False):
    """sources (paths below the repository's root) and nothing else -> the program `out`, by the first of ROCm's clang++, g++ and
    clang++ that builds it"""
    src = [os.path.join(ROOT, s) for s in sources]
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    tried = []
    for cxx in (rocm_clang, shutil.which("g++"), shutil.which("clang++")):
        if not cxx or not os.path.exists(cxx):
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra"] + (SANITIZE if sanitize else []) + ["-o", str(out)] + src + list(libs),
                           capture_output=True, text=True)
        if r.returncode == 0:
            return str(out)
        tried.append("%s:\n%s" % (cxx, r.stderr[-2000:]))
    if skip_without_compiler and not tried:
        pytest.skip("no C++ compiler")
    pytest.fail("no C++ compiler built the program:\n" + "\n".join(tried))


def run(prog, *args, input=None, env_extra=None):
    """the program must end with status 0 and neither sanitizer may have reported (a report also ends it with another status)
    -> the completed process"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **(env_extra or {}))
    r = subprocess.run([prog] + [str(a) for a in args], input=input, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return r
