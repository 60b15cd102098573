"""CPU only: the wide sampler header (csrc/sgp_nuts_wide.hpp, the state machine of the joint NUTS kernel) built with AddressSanitizer
and UndefinedBehaviorSanitizer.  Like tests/test_sanitizers.py it runs its binary without the environment's preloads (the
sanitizer runtime must come first), so it belongs to the CPU container only and is not run on the GPU machines."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "nuts_wide_host.cpp")


def test_wide_sampler_header_is_clean_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "nuts_wide_asan")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    subprocess.run([gxx, "-O1", "-std=c++17", "-DNUTS_HOST_MAIN"] + san + ["-I", INC, "-o", exe, SRC], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "sanitized wide sampler ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
