"""CPU only: the likelihood layer csrc/sgp_lik.hpp built by g++ alone with AddressSanitizer + UBSan as a stand-alone program
(tests/native/lik_host.cpp, its own main) and run: every likelihood function on a grid against long-double quadrature and central
differences, the variance floor, and the overflowing tails.  Sanitizers run on CPU builds only (as in
tests/test_sanitizers.py); this file needs no GPU and, unlike that one, skips itself on a host that has one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_likelihood_layer_on_the_host_under_asan_ubsan(tmp_path):
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on CPU-only hosts, never on a GPU box")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "lik_host_asan")
    subprocess.run([gxx, "-O1", "-std=c++17"] + SAN + ["-I", INC, "-o", exe, os.path.join(ROOT, "tests", "native", "lik_host.cpp")],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "likelihood layer ok" in r.stdout and " 0 failures" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
