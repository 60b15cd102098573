"""Builds libsgp_hip.so (the C-ABI library declared in include/sgp.h) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the resulting
.so travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_NAME = "libsgp_hip.so"
LIB_PATH = os.path.join(CSRC, LIB_NAME)
SOURCES = ["sgp_ctx.hip", "sgp_suffstats_fwd.hip", "sgp_suffstats_i8.hip", "sgp_suffstats_bwd.hip", "sgp_suffstats_bwd_lo.hip", "sgp_dense.hip", "sgp_tail.hip", "sgp_sgpmc.hip", "sgp_sgpmc_lik.hip", "sgp_sgpmc_mc.hip", "sgp_sgpmc_comp.hip", "sgp_svgp.hip", "sgp_svgp_mc.hip", "sgp_composite.hip", "sgp_small.hip", "sgp_exact.hip", "sgp_exact_batch.hip"]
VERSION_SCRIPT = "libsgp.map"
# Companion libraries: (library, sources, public header), in build order.  Each is one more shared object beside libsgp_hip.so with a
# C header of its own, linked to the core library; the core's surface (include/sgp.h) does not grow with them.  A new one is a row here
# and a row of _lib._COMPANION_TABLE.
COMPANIONS = [("libsgp_exact_nuts_hip.so", ["sgp_exact_nuts.hip"], "sgp_exact_nuts.h"),
              ("libsgp_exact_predict_hip.so", ["sgp_exact_predict.hip"], "sgp_exact_predict.h"),
              ("libsgp_vfe_batch_hip.so", ["sgp_vfe_batch.hip"], "sgp_vfe_batch.h"),
              ("libsgp_vfe_nuts_hip.so", ["sgp_vfe_nuts.hip"], "sgp_vfe_nuts.h"),
              ("libsgp_vfe_predict_hip.so", ["sgp_vfe_predict.hip"], "sgp_vfe_predict.h")]
# The companions after the first five, built after them under the same digest rule (a second list: the first is what the earlier
# libraries' tests know as the whole of it)
COMPANIONS_MORE = [("libsgp_mixture_hip.so", ["sgp_mixture.hip"], "sgp_mixture.h")]
PUBLIC_HEADER = os.path.join("..", "..", "include", "sgp.h")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]  # only the SGP_API symbols of include/sgp.h leave the library


def _headers():
    """Every header a translation unit can reach: all of csrc/*.hpp (globbed, so a new #include cannot be forgotten --
    sgp_nuts.hpp once was and the sampler could be edited without a rebuild) plus the public C header."""
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp")) + [PUBLIC_HEADER]
ARCH = "gfx950"


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the sparse-GP core has no CPU fallback and cannot be built without ROCm")


def _digest() -> str:
    h = hashlib.sha256()
    h.update((" ".join(FLAGS) + " " + os.environ.get("SGP_EXTRA_HIPCC_FLAGS", "")).encode())
    for f in SOURCES + _headers() + [VERSION_SCRIPT]:
        h.update(os.path.basename(f).encode())
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _companion_digest(core_digest: str, sources, header) -> str:
    """The core library's digest (flags, every csrc header, the version script) plus the companion's own sources and public header."""
    h = hashlib.sha256(core_digest.encode())
    for f in list(sources) + [os.path.join("..", "..", "include", header)]:
        h.update(os.path.basename(f).encode())
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _compile_and_link(path, sources, digest, force, verbose, parallel=False, to_core=False):
    """Brings the shared object ``path`` up to date with ``digest`` (kept beside it in ``path``.sha256): every source to an object
    file (all at once with ``parallel``), then one link -- ``to_core``: against libsgp_hip.so beside it."""
    stamp = path + ".sha256"
    if not force and os.path.exists(path) and os.path.exists(stamp):
        with open(stamp) as fh:
            if fh.read().strip() == digest:
                return path
    hipcc = _hipcc()
    objs, running = [], []

    def finish(src, proc):
        out, _ = proc.communicate()
        if proc.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, out))
    for src in sources:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        cmd = [hipcc, "--offload-arch=" + ARCH] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        cmd += os.environ.get("SGP_EXTRA_HIPCC_FLAGS", "").split()  # A/B builds (tools/ab_build.sh); empty for the product
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        running.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
        if not parallel:
            finish(*running.pop())
    for job in running:
        finish(*job)
    cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, VERSION_SCRIPT)]
    cmd += (["-Wl,-rpath,$ORIGIN"] if to_core else []) + ["-o", path] + objs + (["-L" + CSRC, "-l:" + LIB_NAME] if to_core else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(("link of %s failed:\n" % os.path.basename(path) if to_core else "link failed:\n") + r.stdout)
    with open(stamp, "w") as fh:
        fh.write(digest)
    return path


def build_companions(force: bool = False, verbose: bool = False):
    """Compile and link every companion library (after the core library, which they link to).  Returns their paths."""
    core = _digest()
    return [_compile_and_link(os.path.join(CSRC, name), sources, _companion_digest(core, sources, header), force, verbose, to_core=True)
            for name, sources, header in COMPANIONS + COMPANIONS_MORE]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP translation unit for gfx950 and link them into csrc/libsgp_hip.so, then the companion libraries."""
    _compile_and_link(LIB_PATH, SOURCES, _digest(), force, verbose, parallel=True)
    build_companions(force, verbose)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
