"""CPU: the batched device-resident NUTS over the exact GP (csrc/sgp_exact_nuts.hip) without a device -- its symbols and host-side
argument checks, the density transform of csrc/sgp_exact_target.hpp against targets.theta_logp_and_grad, the resumable chain under the
host sanitizers, and everything above the engine (sample_exact_nuts_batch, GPR_HMC(device_sampler=True), the experiment's --hmc) on
the CPU double of tests/exact_nuts_double.py, the posterior pin included."""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from exact_nuts_double import BAD_START, ExactNutsDouble

import ggp_amd
import ggp_amd._lib as L
from ggp_amd.hmc import SplitMix
from ggp_amd.targets import in_range, theta_logp_and_grad

T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
CSRC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
NAMES = {"sgp_exact_nuts_batch_workspace_bytes": 3, "sgp_exact_nuts_batch_occupancy": 2, "sgp_exact_nuts_batch_begin": 20,
         "sgp_ctx_exact_nuts_batch_begin": 21, "sgp_exact_nuts_batch_advance": 23, "sgp_ctx_exact_nuts_batch_advance": 24}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load_exact_nuts_library()


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    """The companion library libsgp_exact_nuts_hip.so: include/sgp_exact_nuts.h = its dynamic symbol table = EXACT_NUTS_PROTOTYPES, and
    the core library's surface (include/sgp.h) has none of it."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp_exact_nuts.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sgp_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(L.EXACT_NUTS_PROTOTYPES)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.EXACT_NUTS_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", L.EXACT_NUTS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(NAMES)
    core = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert "sgp_exact_nuts" not in core and not any(n in L.PROTOTYPES for n in NAMES) and L.SGP_ABI_VERSION == 3
    assert hasattr(ggp_amd.HipEngine, "exact_nuts_batch") and L.EXACT_NUTS_BAD_START == BAD_START == 1
    assert "#define SGP_EXACT_NUTS_BAD_START 1" in txt
    import ggp_amd.build as B
    assert ("libsgp_exact_nuts_hip.so", ["sgp_exact_nuts.hip"], "sgp_exact_nuts.h") in B.COMPANIONS
    assert [c[1] for c in B.COMPANIONS].count(["sgp_exact_nuts.hip"]) == 1 and "sgp_exact_nuts.hip" not in B.SOURCES


def test_the_digest_covers_the_companion_library(tmp_path, monkeypatch):
    """build() reuses a companion library while its digest is unchanged: its source, its public header and every csrc header are in it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_sgp_build_en", os.path.join(ROOT, "generalised-gaussian-processes_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    (name, sources, header), = [c for c in b.COMPANIONS if c[0] == "libsgp_exact_nuts_hip.so"]
    before = b._companion_digest(b._digest(), sources, header)
    assert before == open(os.path.join(b.CSRC, name + ".sha256")).read().strip()
    work = tmp_path / "pkg" / "csrc"
    work.mkdir(parents=True)
    for f in os.listdir(b.CSRC):
        if f.endswith((".hip", ".hpp", ".map")):
            shutil.copy(os.path.join(b.CSRC, f), work / f)
    (tmp_path / "include").mkdir()
    for h in ("sgp.h", header):
        shutil.copy(os.path.join(ROOT, "include", h), tmp_path / "include" / h)
    monkeypatch.setattr(b, "CSRC", str(work))
    assert b._companion_digest(b._digest(), sources, header) == before
    for edited in (work / "sgp_exact_nuts.hip", work / "sgp_exact_target.hpp", work / "sgp_nuts.hpp", work / "sgp_wg_dense.hpp",
                   tmp_path / "include" / header):
        with open(edited, "a") as fh:
            fh.write("// a comment\n")
        after = b._companion_digest(b._digest(), sources, header)
        assert after != before, edited
        before = after


def begin(lib, **bad):
    a = dict(q0=8, seed=8, C=4, N=10, d=2, kid=0, tune=5, draws=5, depth=10, step=0.25, accept=0.8, out=8, ws=0, nbytes=0)
    a.update(bad)
    p = lambda k: C.c_void_p(a[k])  # noqa: E731  (the dummy 8 is never dereferenced: every call here fails validation first)
    return lib.sgp_exact_nuts_batch_begin(p("q0"), p("seed"), a["C"], a["N"], a["d"], a["kid"], a["tune"], a["draws"], a["depth"], a["step"],
                                          a["accept"], p("out"), p("out"), p("out"), p("out"), p("out"), p("out"), p("ws"), a["nbytes"], None)


def advance(lib, **bad):
    a = dict(X=8, Y=8, C=4, N=10, d=2, ldx=2, kid=0, jitter=0.0, out=8, epl=16, fin=1, ws=0, nbytes=0)
    a.update(bad)
    p = lambda k: C.c_void_p(a[k])  # noqa: E731
    fin = C.c_int64(-7)
    st = lib.sgp_exact_nuts_batch_advance(p("X"), a["N"] * a["d"], a["ldx"], p("Y"), a["N"], None, None, a["C"], a["N"], a["d"], a["kid"],
                                          a["jitter"], p("out"), p("out"), p("out"), p("out"), p("out"), p("out"), a["epl"],
                                          C.byref(fin) if a["fin"] else None, p("ws"), a["nbytes"], None)
    assert fin.value == -7  # nothing ran
    return st


ROWS = [  # (what is wrong, status): SGP_ERR_ARG = -1 before SGP_ERR_DIM = -2 before SGP_ERR_WORKSPACE = -3, all before any launch
    (dict(N=129), -2), (dict(d=9, ldx=9), -2), (dict(C=0), -1), (dict(C=2 ** 24), -2), (dict(kid=3), -1), (dict(kid=-1), -1),
    (dict(N=0), -1), (dict(), -3), (dict(ws=8, nbytes=255), -3), (dict(ws=0, nbytes=1 << 40), -3),
    (dict(N=129, kid=3), -1), (dict(N=129, out=0), -1), (dict(N=129, ws=8, nbytes=1 << 40), -2), (dict(out=0), -1),
]


def test_argument_checks_need_no_device(lib):
    for bad, want in ROWS:
        assert begin(lib, **bad) == want, ("begin", bad)
        assert advance(lib, **bad) == want, ("advance", bad)
    for bad, want in [(dict(depth=12), -1), (dict(depth=-1), -1), (dict(q0=0), -1), (dict(seed=0), -1), (dict(tune=-1), -1),
                      (dict(step=0.0), -1), (dict(accept=1.0), -1), (dict(depth=12, N=129), -1), (dict(depth=11), -3)]:
        assert begin(lib, **bad) == want, ("begin", bad)
    for bad, want in [(dict(X=0), -1), (dict(Y=0), -1), (dict(fin=0), -1), (dict(epl=0), -1), (dict(ldx=1), -1), (dict(jitter=-1.0), -1),
                      (dict(jitter=float("nan")), -1)]:
        assert advance(lib, **bad) == want, ("advance", bad)
    q = lib.sgp_exact_nuts_batch_workspace_bytes
    for shape in [(4, 129, 1), (4, 10, 9), (0, 10, 1), (2 ** 24, 10, 2), (4, 0, 1), (4, 10, 0)]:
        assert q(*shape) == 0, shape
    assert 0 < q(1, 1, 1) < q(2, 128, 8) < q(2 ** 24 - 1, 10, 2)
    assert q(3, 10, 2) - q(2, 10, 2) == q(2, 10, 2) - q(1, 10, 2) >= 18992  # one sampler state per chain
    assert lib.sgp_exact_nuts_batch_occupancy(129, 0) == -2 and lib.sgp_exact_nuts_batch_occupancy(10, 3) == -1
    assert lib.sgp_exact_nuts_batch_occupancy(0, 0) == -1


# ---------------------------------------------------------------------------------------------------------------- 3: the transform
@pytest.fixture(scope="module")
def target_lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("ext") / "libexact_target_host.so")
    # -ffp-contract=off: no fused multiply-adds the Python arithmetic does not have
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "native", "exact_target_host.cpp")], check=True, timeout=300)
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.ext_host_in_range.restype, lib.ext_host_in_range.argtypes = C.c_int, [dp, C.c_int]
    lib.ext_host_constrain.restype, lib.ext_host_constrain.argtypes = None, [dp, C.c_int, C.c_double, dp, dp]
    lib.ext_host_logp_grad.restype, lib.ext_host_logp_grad.argtypes = C.c_double, [dp, C.c_int, C.c_double, dp, C.c_int, dp]
    return lib


def arr(v):
    return (C.c_double * len(v))(*[float(t) for t in v])


def host_eval(tl, q, F, g, info=0):
    d = len(q) - 2
    grad = (C.c_double * (d + 2))()
    return tl.ext_host_logp_grad(arr(q), d, float(F), arr(g), info, grad), list(grad)


def python_eval(q, F, g, info=0):
    """ExactHmcTarget._eval after the evaluation."""
    q = [float(v) for v in q]
    d = len(q) - 2
    if not in_range(q) or info != 0 or not math.isfinite(F):
        return -math.inf, [0.0] * (d + 2)
    v = [math.exp(t) for t in q]
    return theta_logp_and_grad(q, v[:d], v[d], v[d + 1], float(F), [float(t) for t in g[:d]], float(g[d]), float(g[d + 1]), finite_grad=True)


@pytest.mark.parametrize("d", [1, 3, 8])
def test_transform_header_against_theta_logp_and_grad(target_lib, d):
    rng = np.random.default_rng(100 + d)
    close = lambda a, b: abs(a - b) <= 1e-14 * abs(b)  # noqa: E731
    for _ in range(200):
        q, F, g = 1.5 * rng.standard_normal(d + 2), 50.0 * rng.standard_normal(), 10.0 * rng.standard_normal(d + 2)
        lp, grad = host_eval(target_lib, q, F, g)
        lp_ref, grad_ref = python_eval(q, F, g)
        assert math.isfinite(lp_ref) and close(lp, lp_ref), (q, lp, lp_ref)
        assert all(close(a, b) for a, b in zip(grad, grad_ref)), (q, grad, grad_ref)
        v, th = (C.c_double * (d + 2))(), (C.c_double * (d + 2))()
        target_lib.ext_host_constrain(arr(q), d, 1e-3, v, th)
        e = [math.exp(t) for t in q]
        assert list(v) == e and list(th) == e[:d] + [e[d] * e[d], e[d + 1] * e[d + 1] + 1e-3]


def test_transform_header_at_the_edges(target_lib):
    d = 3
    q, g = [0.1, -0.2, 0.3, 0.4, -0.5], [1.0, -2.0, 3.0, 0.5, -0.25]
    for k, bad in [(0, 300.0), (4, -300.0), (2, float("nan")), (3, float("inf")), (1, -float("inf")), (4, 1e308)]:
        p = list(q)
        p[k] = bad
        assert target_lib.ext_host_in_range(arr(p), d + 2) == 0 and not in_range(p)
    for k, ok in [(0, 299.999), (4, -299.999), (2, 0.0)]:
        p = list(q)
        p[k] = ok
        assert target_lib.ext_host_in_range(arr(p), d + 2) == 1 and in_range(p)
    zeros = [0.0] * (d + 2)
    for k in range(d + 2):  # a non-finite gradient entry: (-inf, zeros)
        for bad in (float("inf"), -float("inf"), float("nan")):
            gg = list(g)
            gg[k] = bad
            assert host_eval(target_lib, q, -3.0, gg) == (-math.inf, zeros) == python_eval(q, -3.0, gg)
    assert host_eval(target_lib, q, -3.0, g, info=7) == (-math.inf, zeros) == python_eval(q, -3.0, g, info=7)   # a failed factorisation
    for F in (float("nan"), float("inf"), -float("inf")):
        assert host_eval(target_lib, q, F, g) == (-math.inf, zeros) == python_eval(q, F, g)
    big = [250.0, 0.0, 0.0, 0.0, 0.0]  # in range, but exp(250) (1 / v - 1 + g) overflows nothing; the density is finite there
    assert host_eval(target_lib, big, -3.0, g)[0] == python_eval(big, -3.0, g)[0]


# ---------------------------------------------------------------------------------------------------------------- 4: save / resume
def test_resumable_chain_under_the_host_sanitizers(tmp_path):
    """A stand-alone program (its own main; nothing is loaded into Python) built with -fsanitize=address,undefined."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on CPU-only hosts, never on a GPU box")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "exact_nuts_resume")
    subprocess.run([gxx, "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "native", "exact_nuts_resume.cpp")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    runs = [subprocess.run([exe, str(chunk)], capture_output=True, text=True, timeout=300, env=env) for chunk in (0, 3)]
    for r in runs:
        assert r.returncode == 0, r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "resumes 0" in runs[0].stderr and "resumes 0" not in runs[1].stderr
    lines = runs[0].stdout.splitlines()
    assert len(lines) == 51 and lines[0].endswith("draws 80") and int(lines[0].split()[1]) > 80
    assert runs[0].stdout == runs[1].stdout


# ---------------------------------------------------------------------------------------------------------------- 5: on the double
def toy(B=2, N=12, d=1, seed=0):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-3.0, 3.0, (N, d)), 0)
    Y = np.sin(X.sum(1))[None] + 0.2 * rng.standard_normal((B, N))
    return X, Y


def test_trace_surface_and_raw_arrays():
    X, Y = toy()
    eng = ExactNutsDouble()
    r = ggp_amd.sample_exact_nuts_batch(X, Y, 6, 8, chains=2, seed=3, engine=eng)
    assert isinstance(r, ggp_amd.ExactNutsResult) and eng.calls["exact_nuts_batch"] == 1
    assert r.samples.shape == (2, 2, 6, 3) and r.stats.shape == (2, 2, 6, 8) and r.seconds.shape == (2, 2, 6)
    assert r.evaluations.shape == r.draws.shape == r.info.shape == r.seeds.shape == (2, 2) and r.starts.shape == (2, 2, 3)
    assert (r.info == 0).all() and (r.draws == 14).all() and r.posterior_mean().shape == (2, 3)
    for b in range(2):
        for c in range(2):
            tr = r.traces[b][c]
            assert isinstance(tr, ggp_amd.Trace) and len(tr) == 6 and set(tr.varnames) == {"ls", "sig_f", "sig_n"}
            assert np.asarray(tr["ls"]).shape == (6, 1) and np.asarray(tr["sig_f"]).shape == (6,)
            assert np.array_equal(np.stack([row["theta_unc"] for row in tr]), r.samples[b, c])
            assert np.allclose(np.log(tr["sig_n"]), r.samples[b, c, :, 2], rtol=0.0, atol=1e-14)
            assert np.array_equal(tr.get_sampler_stats("step_size"), r.stats[b, c, :, 0])
            assert tr.get_sampler_stats("diverging").dtype == bool and tr.get_sampler_stats("perf_counter_diff").shape == (6,)
            assert {"tree_size", "depth", "mean_tree_accept", "energy", "logp"} <= tr.stat_names
            assert tr.n_leapfrog == r.evaluations[b, c] == r.stats[b, c, -1, 7] and tr.device_resident
            assert len(tr[2:5]) == 3 and ggp_amd.models.trace_summary(tr)[1] == [r.stats[b, c, 0, 0]]
    with pytest.raises(ValueError):
        ggp_amd.sample_exact_nuts_batch(np.zeros((129, 1)), np.zeros((1, 129)), 2, 2, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.sample_exact_nuts_batch(X, Y, 2, 2, kernel="composite", engine=eng)


def test_a_chain_alone_is_the_chain_in_a_batch():
    X, Y = toy(B=3)
    r = ggp_amd.sample_exact_nuts_batch(X, Y, 5, 6, chains=2, seed=11, engine=ExactNutsDouble())
    for b in range(3):
        for c in range(2):  # the documented rule: it depends on (seed, b, c) alone
            s = SplitMix(11)
            for _ in range(b + 1):
                sb = s._u64()
            s = SplitMix(sb)
            for _ in range(c + 1):
                sc = s._u64()
            assert int(r.seeds[b, c]) == ggp_amd.chain_seed(11, b, c) == sc
    assert len(set(r.seeds.reshape(-1).tolist())) == 6
    one = ggp_amd.sample_exact_nuts_batch(X, Y[2], 5, 6, chains=1, seeds=[[int(r.seeds[2, 1])]], engine=ExactNutsDouble())
    assert np.array_equal(one.samples[0, 0], r.samples[2, 1]) and np.array_equal(one.stats[0, 0], r.stats[2, 1])
    assert np.array_equal(one.starts[0, 0], r.starts[2, 1]) and one.evaluations[0, 0] == r.evaluations[2, 1]
    wide = ggp_amd.sample_exact_nuts_batch(X, Y[:2], 5, 6, chains=3, seed=11, engine=ExactNutsDouble())   # another batch around (1, 1)
    assert np.array_equal(wide.samples[1, 1], r.samples[1, 1])
    ard = np.stack([X, X[::-1]])  # one X per data set
    two = ggp_amd.sample_exact_nuts_batch(ard, Y[:2], 4, 4, seed=5, engine=ExactNutsDouble())
    rev = ggp_amd.sample_exact_nuts_batch(X[::-1], Y[1], 4, 4, seeds=[[int(two.seeds[1, 0])]], engine=ExactNutsDouble())
    assert np.array_equal(two.samples[1, 0], rev.samples[0, 0])


class ZeroDensityAtFirst(ExactNutsDouble):
    """The double, except that the first ``rounds`` value-only batches report chain ``who`` as not positive definite."""

    def __init__(self, who, rounds):
        super().__init__()
        self.who, self.rounds, self.value_only, self.seeds_seen = who, rounds, 0, None

    def exact_eval_batch(self, X, Y, theta, ix=None, iy=None, kernel="rbf", want_grad=True):
        F, out, g, info = super().exact_eval_batch(X, Y, theta, ix, iy, kernel, want_grad)
        if not want_grad:
            self.value_only += 1
            if self.value_only <= self.rounds:
                info[self.who] = 3
                out[self.who] = float("nan")
        return out[:, 0], out, g, info

    def exact_nuts_batch(self, X, Y, q0, seeds, *a, **kw):
        self.seeds_seen = [int(s) for s in seeds]
        return super().exact_nuts_batch(X, Y, q0, seeds, *a, **kw)


def test_start_redraw_and_the_user_start():
    X, Y = toy(B=3)
    base = np.array([math.log(2.0), 0.0, 0.0])
    eng = ZeroDensityAtFirst(who=1, rounds=2)
    r = ggp_amd.sample_exact_nuts_batch(X, Y, 3, 3, seed=4, engine=eng)
    assert eng.value_only == 3 and (r.info == 0).all()   # two rounds with a bad chain, the third finds none
    for b in range(3):  # hmc._find_start: test point + U(-1, 1) from the chain's own SplitMix, redrawn for the chain that failed alone
        s = SplitMix(ggp_amd.chain_seed(4, b, 0))
        draws = [base + s.uniform(-1.0, 1.0, 3) for _ in range(3 if b == 1 else 1)]
        assert np.array_equal(r.starts[b, 0], draws[-1]) and eng.seeds_seen[b] == s.s   # the sampler continues that stream
    never = ZeroDensityAtFirst(who=0, rounds=10 ** 6)   # the density never becomes finite: 1 + 20 draws, then the chain is left to report
    r = ggp_amd.sample_exact_nuts_batch(X, Y[:1], 3, 3, seed=4, engine=never)
    assert never.value_only == 20 and (r.info == 0).all()
    # a user-supplied start is never replaced, never pre-checked
    eng = ZeroDensityAtFirst(who=1, rounds=5)
    q = np.array([0.3, 0.2, -0.4])
    r = ggp_amd.sample_exact_nuts_batch(X, Y, 3, 3, seed=4, start=q, engine=eng)
    assert eng.value_only == 0 and (r.starts == q).all() and eng.seeds_seen == [ggp_amd.chain_seed(4, b, 0) for b in range(3)]
    per = np.stack([q + 0.1 * b for b in range(3)])[:, None, :]
    r2 = ggp_amd.sample_exact_nuts_batch(X, Y, 3, 3, seed=4, start=per, engine=ExactNutsDouble())
    assert np.array_equal(r2.starts, per) and np.array_equal(r2.samples[0], r.samples[0]) and not np.array_equal(r2.samples[1], r.samples[1])


def test_info_of_a_bad_start():
    X, Y = toy(B=3)
    start = np.tile(np.array([0.3, 0.2, -0.4]), (3, 2, 1))
    start[0, 1, 0] = float("nan")
    start[2, 0, 2] = 300.0
    r = ggp_amd.sample_exact_nuts_batch(X, Y, 4, 4, chains=2, seed=9, start=start, engine=ExactNutsDouble())
    bad = np.zeros((3, 2), dtype=bool)
    bad[0, 1] = bad[2, 0] = True
    assert np.array_equal(r.info, np.where(bad, L.EXACT_NUTS_BAD_START, 0))
    assert np.isnan(r.samples[bad]).all() and np.isnan(r.stats[bad]).all() and np.isnan(r.seconds[bad]).all()
    assert np.isfinite(r.samples[~bad]).all() and (r.draws[bad] == 0).all() and (r.draws[~bad] == 8).all()
    good = ggp_amd.sample_exact_nuts_batch(X, Y, 4, 4, chains=2, seed=9, start=np.array([0.3, 0.2, -0.4]), engine=ExactNutsDouble())
    assert np.array_equal(good.samples[~bad], r.samples[~bad])
    assert np.isfinite(r.posterior_mean()).all()


def _model(device_sampler, N=60, d=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    eng = ExactNutsDouble()
    kw = {"device_sampler": True} if device_sampler else {}
    return ggp_amd.GPR_HMC(T(X), T(y), ggp_amd.GaussianLikelihood(), engine=eng, seed=1, **kw), eng, X


def test_gpr_hmc_device_sampler_is_opt_in():
    m, eng, X = _model(True)
    trace, step, perf = m.train_model()
    assert eng.calls["exact_nuts_batch"] == 1 and eng.calls["exact_eval"] == 0
    assert len(trace) == 10 and np.asarray(trace["ls"]).shape == (10, 2) and trace.device_resident
    assert len(step) == 1 and step[0] > 0 and len(perf) == 1
    assert ggp_amd.full_mixture_posterior_predictive(m, T(X[:7]), trace) is not None and eng.calls["exact_predict"] >= 1
    again = m.sample_optimal_variational_hyper_dist(3, 2, 4)   # the model's next seed, as on the host path
    assert len(again) == 3 and eng.calls["exact_nuts_batch"] == 2
    # the default model does not touch the new path ...
    m0, eng0, _ = _model(False)
    trace0, _, _ = m0.train_model()
    assert eng0.calls["exact_nuts_batch"] == 0 and eng0.calls["exact_eval"] > 0 and not hasattr(trace0, "device_resident")
    # ... and neither does an opted-in model beyond the device sampler's size (N <= 128)
    m1, eng1, _ = _model(True, N=130)
    m1.sample_optimal_variational_hyper_dist(2, 2, 2)
    assert eng1.calls["exact_nuts_batch"] == 0 and eng1.calls["exact_eval"] > 0


def test_experiment_hmc_flag_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    eng = ExactNutsDouble()
    s = mod.main(["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4", "--out", str(tmp_path), "--hmc", "--hmc_chains", "2",
                  "--hmc_tune", "8", "--hmc_draws", "6"], engine=eng)
    assert eng.calls["exact_nuts_batch"] == 2   # one batch per cell: the size cell and the noise cell
    z = np.load(tmp_path / "hyperparameter_identification.npz")
    for name in ("size", "noise"):
        for k in ("log_ls", "log_sf", "log_sn"):
            assert z["%s_hmc_%s" % (name, k)].shape == (1, 2) == z["%s_learn_ls" % name].shape and np.isfinite(z["%s_hmc_%s" % (name, k)]).all()
            assert s["%s_hmc_mean_%s" % (name, k)] == [float(z["%s_hmc_%s" % (name, k)].mean())]
        assert 0.0 <= s["%s_hmc_diverging" % name][0] <= 1.0
    assert "size_hmc_mean_log_ls" in json.load(open(tmp_path / "hyperparameter_identification.json"))
    # off by default: nothing of it in the outputs
    eng = ExactNutsDouble()
    s = mod.main(["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4", "--out", str(tmp_path / "plain")], engine=eng)
    assert eng.calls["exact_nuts_batch"] == 0 and not any("hmc" in k for k in s)


# ---------------------------------------------------------------------------------------------------------------- 6: the posterior pin
PIN_SEED = 1


def pin_run(engine):
    """8 chains x (400 tune + 150 draws) on pin_data(), pooled: (draws x 3, share of diverging draws)."""
    from test_gpr_hmc import pin_data
    X, y = pin_data()
    r = ggp_amd.sample_exact_nuts_batch(X, y, 150, 400, chains=8, seed=PIN_SEED, engine=engine)
    assert (r.info == 0).all() and (r.draws == 550).all()
    return r.samples.reshape(-1, 3), float(r.stats[..., 4].mean())


def test_quadrature_posterior_pin_on_the_double():
    from test_gpr_hmc import pin_data, quadrature_posterior
    from test_posterior_pin import check_moments
    th, diverging = pin_run(ExactNutsDouble())
    assert diverging <= 0.01
    check_moments(th, quadrature_posterior(*pin_data()), "sample_exact_nuts_batch / double")
