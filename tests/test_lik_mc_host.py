"""CPU only: ``lik_robustmax`` of csrc/sgp_lik.hpp built by g++ alone as a stand-alone program (tests/native/lik_mc_host.cpp, its own
main) and run: the likelihood on a grid of C in {2, 3, 16}, |mu| up to 40 and var from the floor to 100 against the long-double
quadrature and its central differences, ties, saturated data and labels that are no class.  On a host without a GPU the program is
built with AddressSanitizer + UBSan (sanitizers run on CPU builds only, as in tests/test_lik_host.py); on a GPU box without them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_robustmax_on_the_host_against_long_double(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    san = [] if os.path.exists("/dev/kfd") else SAN
    exe = str(tmp_path / "lik_mc_host")
    subprocess.run([gxx, "-O1", "-std=c++17"] + san + ["-I", INC, "-o", exe, os.path.join(ROOT, "tests", "native", "lik_mc_host.cpp")],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "robust-max layer ok" in r.stdout and " 0 failures" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
