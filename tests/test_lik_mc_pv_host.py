"""CPU only: ``lik_robustmax_pv`` of csrc/sgp_lik.hpp (the robust-max likelihood with one variance per class, what the multi-class SVGP
bound evaluates per datum) built by g++ alone as a stand-alone program (tests/native/lik_mc_pv_host.cpp, its own main) and run: a grid of
C in {2, 3, 16}, |mu| up to 40 and per-class variances from the floor to 100, equal, independent and a factor 1e6 apart, against the
long-double quadrature and its central differences; ties, saturated data, variances below the floor, labels that are no class, the strided
layout of the device, and the identity with ``lik_robustmax`` at equal variances.  On a host without a GPU the program is built with
AddressSanitizer + UBSan (sanitizers run on CPU builds only, as in tests/test_lik_mc_host.py); on a GPU box without them.  The program
runs in the environment as it is."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_robustmax_per_class_variance_on_the_host_against_long_double(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    san = [] if os.path.exists("/dev/kfd") else SAN
    exe = str(tmp_path / "lik_mc_pv_host")
    subprocess.run([gxx, "-O1", "-std=c++17"] + san + ["-I", INC, "-o", exe, os.path.join(ROOT, "tests", "native", "lik_mc_pv_host.cpp")],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "robust-max per-class-variance layer ok" in r.stdout and " 0 failures" in r.stdout, \
        (r.stdout[-3000:], r.stderr[-3000:])
