"""CPU: the batched device-resident NUTS over the collapsed sparse-GP bound (csrc/sgp_vfe_nuts.hip) without a device -- its symbols and
host-side argument checks, and everything above the engine (sample_sgpr_nuts_batch, SgprBatchResult.sample_nuts, SgprNutsResult.model,
the experiment's --sparse M --hmc) on the CPU double of tests/vfe_nuts_double.py, the posterior pin included."""
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

from conftest import ROOT, load_golden
from vfe_nuts_double import BAD_START, VfeNutsDouble

import ggp_amd
import ggp_amd._lib as L
from ggp_amd.hmc import SplitMix

T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
CSRC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
NAMES = {"sgp_vfe_nuts_batch_workspace_bytes": 4, "sgp_vfe_nuts_batch_occupancy": 2, "sgp_vfe_nuts_batch_begin": 21,
         "sgp_ctx_vfe_nuts_batch_begin": 22, "sgp_vfe_nuts_batch_advance": 28, "sgp_ctx_vfe_nuts_batch_advance": 29}
ENTRY = ("libsgp_vfe_nuts_hip.so", ["sgp_vfe_nuts.hip"], "sgp_vfe_nuts.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load_vfe_nuts_library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    """The companion library libsgp_vfe_nuts_hip.so: include/sgp_vfe_nuts.h = its dynamic symbol table = VFE_NUTS_PROTOTYPES, and neither
    the core library's surface (include/sgp.h) nor another companion's table has any of it."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp_vfe_nuts.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sgp_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(L.VFE_NUTS_PROTOTYPES)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.VFE_NUTS_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", L.VFE_NUTS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(NAMES)
    und = subprocess.run([nm, "-D", "--undefined-only", L.VFE_NUTS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert [ln.split()[-1] for ln in und.splitlines() if re.search(r"\bsgp_", ln)] == ["sgp_ctx_device"]   # all it takes from the core
    core = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert "sgp_vfe_nuts" not in core and L.SGP_ABI_VERSION == 3 and len(L.PROTOTYPES) == 146
    for table in (L.PROTOTYPES, L.EXACT_NUTS_PROTOTYPES, L.EXACT_PREDICT_PROTOTYPES, L.VFE_BATCH_PROTOTYPES):
        assert not any(n in table for n in NAMES)
    assert L._COMPANION_TABLE["vfe_nuts"] == (L.VFE_NUTS_LIB_PATH, L.VFE_NUTS_PROTOTYPES)
    assert hasattr(ggp_amd.HipEngine, "vfe_nuts_batch") and hasattr(ggp_amd.HipEngine, "vfe_nuts_evals_per_launch")
    assert L.VFE_NUTS_BAD_START == BAD_START == 1 and "#define SGP_VFE_NUTS_BAD_START 1" in txt
    import ggp_amd.build as B
    assert B.COMPANIONS.count(ENTRY) == 1
    assert [c[1] for c in B.COMPANIONS].count(["sgp_vfe_nuts.hip"]) == 1 and "sgp_vfe_nuts.hip" not in B.SOURCES


def test_the_digest_covers_the_new_library(lib, tmp_path, monkeypatch):
    """build() reuses the library while its digest is unchanged: its source, its public header and every csrc header are in it."""
    spec = importlib.util.spec_from_file_location("_sgp_build_vn", os.path.join(ROOT, "generalised-gaussian-processes_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    (name, sources, header), = [c for c in b.COMPANIONS if c[0] == "libsgp_vfe_nuts_hip.so"]
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
    for edited in (work / "sgp_vfe_nuts.hip", work / "sgp_vfe_batch.hpp", work / "sgp_exact_target.hpp", work / "sgp_nuts.hpp",
                   work / "sgp_wg_dense.hpp", tmp_path / "include" / header):
        with open(edited, "a") as fh:
            fh.write("// a comment\n")
        after = b._companion_digest(b._digest(), sources, header)
        assert after != before, edited
        before = after


# ---------------------------------------------------------------------------------------------------------------- refusals, no device
def begin(lib, ctx=False, **bad):
    a = dict(q0=8, seed=8, C=4, N=10, M=5, d=2, kid=0, tune=5, draws=5, depth=10, step=0.25, accept=0.8, out=8, ws=0, nbytes=0)
    a.update(bad)
    p = lambda k: C.c_void_p(a[k])  # noqa: E731  (the dummy 8 is never dereferenced: every call here fails validation first)
    args = (p("q0"), p("seed"), a["C"], a["N"], a["M"], a["d"], a["kid"], a["tune"], a["draws"], a["depth"], a["step"], a["accept"],
            p("out"), p("out"), p("out"), p("out"), p("out"), p("out"), p("ws"), a["nbytes"], None)
    return lib.sgp_ctx_vfe_nuts_batch_begin(None, *args) if ctx else lib.sgp_vfe_nuts_batch_begin(*args)


def advance(lib, ctx=False, **bad):
    a = dict(X=8, Y=8, Z=8, C=4, N=10, M=5, d=2, ldx=2, ldz=2, kid=0, jitter=1e-6, out=8, epl=16, fin=1, ws=0, nbytes=0)
    a.update(bad)
    p = lambda k: C.c_void_p(a[k])  # noqa: E731
    fin = C.c_int64(-7)
    args = (p("X"), a["N"] * a["d"], a["ldx"], p("Y"), a["N"], None, None, p("Z"), a["M"] * a["d"], a["ldz"], None, a["C"], a["N"], a["M"],
            a["d"], a["kid"], a["jitter"], p("out"), p("out"), p("out"), p("out"), p("out"), p("out"), a["epl"],
            C.byref(fin) if a["fin"] else None, p("ws"), a["nbytes"], None)
    st = lib.sgp_ctx_vfe_nuts_batch_advance(None, *args) if ctx else lib.sgp_vfe_nuts_batch_advance(*args)
    assert fin.value == -7  # nothing ran
    return st


ROWS = [  # (what is wrong, status): SGP_ERR_ARG = -1 before SGP_ERR_DIM = -2 before SGP_ERR_WORKSPACE = -3, all before any launch
    (dict(M=65), -2), (dict(N=65537), -2), (dict(d=9, ldx=9, ldz=9), -2), (dict(C=2 ** 24), -2), (dict(kid=3), -1), (dict(kid=-1), -1),
    (dict(C=0), -1), (dict(N=0), -1), (dict(M=0), -1), (dict(d=0), -1), (dict(), -3), (dict(ws=8, nbytes=255), -3),
    (dict(ws=0, nbytes=1 << 40), -3), (dict(N=3, M=5), -3),   # M > N is legal: it gets as far as the workspace
    (dict(M=65, kid=3), -1), (dict(M=65, out=0), -1), (dict(N=65537, out=0), -1), (dict(M=65, ws=8, nbytes=1 << 40), -2), (dict(out=0), -1),
]


def test_argument_checks_need_no_device(lib):
    for ctx in (False, True):
        for bad, want in ROWS:
            assert begin(lib, ctx, **bad) == want, ("begin", ctx, bad)
            assert advance(lib, ctx, **bad) == want, ("advance", ctx, bad)
        for bad, want in [(dict(depth=12), -1), (dict(depth=-1), -1), (dict(q0=0), -1), (dict(seed=0), -1), (dict(tune=-1), -1),
                          (dict(draws=-1), -1), (dict(step=0.0), -1), (dict(accept=1.0), -1), (dict(depth=12, M=65), -1), (dict(depth=11), -3)]:
            assert begin(lib, ctx, **bad) == want, ("begin", ctx, bad)
        for bad, want in [(dict(X=0), -1), (dict(Y=0), -1), (dict(Z=0), -1), (dict(fin=0), -1), (dict(epl=0), -1), (dict(epl=-3), -1),
                          (dict(ldx=1), -1), (dict(ldz=1), -1), (dict(jitter=-1e-6), -1), (dict(jitter=float("nan")), -1),
                          (dict(epl=0, N=65537), -1), (dict(jitter=-1.0, ws=8, nbytes=1 << 40), -1), (dict(jitter=0.0), -3)]:
            assert advance(lib, ctx, **bad) == want, ("advance", ctx, bad)
    q = lib.sgp_vfe_nuts_batch_workspace_bytes
    for shape in [(4, 10, 65, 1), (4, 65537, 5, 1), (4, 10, 5, 9), (0, 10, 5, 1), (2 ** 24, 10, 5, 2), (4, 0, 5, 1), (4, 10, 0, 1), (4, 10, 5, 0)]:
        assert q(*shape) == 0, shape
    assert 0 < q(1, 1, 1, 1) < q(2, 65536, 64, 8) < q(2 ** 24 - 1, 10, 5, 2) and q(2, 3, 5, 1) > 0 and q(1, 1, 1, 1) % 256 == 0
    per_chain = (q(1280, 10, 5, 2) - q(256, 10, 5, 2)) / 1024   # one sampler state, a theta row, an out row and an info word per chain
    assert per_chain >= 18992 + 8 * (4 + 7) + 4 and q(1280, 10, 5, 8) > q(1280, 10, 5, 2)
    occ = lib.sgp_vfe_nuts_batch_occupancy
    assert occ(65, 0) == -2 and occ(10, 3) == -1 and occ(0, 0) == -1 and occ(65, 3) == -1


# ---------------------------------------------------------------------------------------------------------------- on the double
def toy(B=2, N=12, d=1, M=4, seed=0):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-3.0, 3.0, (N, d)), 0)
    Y = np.sin(X.sum(1))[None] + 0.2 * rng.standard_normal((B, N))
    Z = X[np.round(np.linspace(0, N - 1, M)).astype(int)].copy()
    return X, Y, Z


def test_trace_surface_and_raw_arrays():
    X, Y, Z = toy()
    eng = VfeNutsDouble()
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 6, 8, chains=2, seed=3, engine=eng)
    assert isinstance(r, ggp_amd.SgprNutsResult) and eng.calls["vfe_nuts_batch"] == 1
    assert r.samples.shape == (2, 2, 6, 3) and r.stats.shape == (2, 2, 6, 8) and r.seconds.shape == (2, 2, 6)
    assert r.evaluations.shape == r.draws.shape == r.info.shape == r.seeds.shape == (2, 2) and r.starts.shape == (2, 2, 3)
    assert (r.info == 0).all() and (r.draws == 14).all() and r.posterior_mean().shape == (2, 3)
    assert np.array_equal(r.X, X) and np.array_equal(r.Y, Y) and np.array_equal(r.Z, Z) and r.kernel == "rbf" and r.jitter == 1e-6
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
    # the logp column is HmcTarget's density at the draw: the jitter on K_uu, not on the noise
    q = r.samples[1, 0, 3]
    assert r.stats[1, 0, 3, 6] == eng.vfe_logp_and_grad(T(X), T(Y[1]), T(Z), q)[0]
    with pytest.raises(ValueError, match="M <= 64"):
        ggp_amd.sample_sgpr_nuts_batch(X, Y, np.zeros((65, 1)), 2, 2, engine=eng)
    with pytest.raises(ValueError, match="N <= 65536"):
        ggp_amd.sample_sgpr_nuts_batch(np.zeros((65537, 1)), np.zeros((1, 65537)), Z, 2, 2, engine=eng)
    with pytest.raises(ValueError, match="d <= 8"):
        ggp_amd.sample_sgpr_nuts_batch(np.zeros((12, 9)), Y, np.zeros((4, 9)), 2, 2, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 2, 2, kernel="composite", engine=eng)
    assert eng.calls["vfe_nuts_batch"] == 1


def test_a_chain_alone_is_the_chain_in_a_batch():
    X, Y, Z = toy(B=3)
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 5, 6, chains=2, seed=11, engine=VfeNutsDouble())
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
    one = ggp_amd.sample_sgpr_nuts_batch(X, Y[2], Z, 5, 6, chains=1, seeds=[[int(r.seeds[2, 1])]], engine=VfeNutsDouble())
    assert np.array_equal(one.samples[0, 0], r.samples[2, 1]) and np.array_equal(one.stats[0, 0], r.stats[2, 1])
    assert np.array_equal(one.starts[0, 0], r.starts[2, 1]) and one.evaluations[0, 0] == r.evaluations[2, 1]
    wide = ggp_amd.sample_sgpr_nuts_batch(X, Y[:2], Z, 5, 6, chains=3, seed=11, engine=VfeNutsDouble())   # another batch around (1, 1)
    assert np.array_equal(wide.samples[1, 1], r.samples[1, 1])


def test_shared_and_per_set_inputs():
    X, Y, Z = toy(B=2)
    Xs, Zs = np.stack([X, X[::-1]]), np.stack([Z, Z[::-1] + 0.05])   # one X and one Z per data set
    two = ggp_amd.sample_sgpr_nuts_batch(Xs, Y, Zs, 4, 4, seed=5, engine=VfeNutsDouble())
    assert two.Z.shape == (2, 4, 1) and two.X.shape == (2, 12, 1)
    alone = ggp_amd.sample_sgpr_nuts_batch(Xs[1], Y[1], Zs[1], 4, 4, seeds=[[int(two.seeds[1, 0])]], engine=VfeNutsDouble())
    assert np.array_equal(two.samples[1, 0], alone.samples[0, 0])
    shared = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 4, 4, seed=5, engine=VfeNutsDouble())
    assert np.array_equal(shared.samples[0, 0], two.samples[0, 0]) and not np.array_equal(shared.samples[1, 0], two.samples[1, 0])
    with pytest.raises(ValueError, match="Z must be"):
        ggp_amd.sample_sgpr_nuts_batch(X, Y, np.stack([Z] * 3), 2, 2, engine=VfeNutsDouble())


class ZeroDensityAtFirst(VfeNutsDouble):
    """The double, except that the first ``rounds`` value-only batches report chain ``who`` as not positive definite."""

    def __init__(self, who, rounds):
        super().__init__()
        self.who, self.rounds, self.value_only, self.seeds_seen = who, rounds, 0, None

    def vfe_eval_batch(self, X, Y, Z, theta, ix=None, iy=None, iz=None, kernel="rbf", jitter=1e-6, want_grad=True, want_gz=False):
        out, gz, info = super().vfe_eval_batch(X, Y, Z, theta, ix, iy, iz, kernel, jitter, want_grad, want_gz)
        if not want_grad:
            self.value_only += 1
            if self.value_only <= self.rounds:
                info[self.who] = 3
                out[self.who] = float("nan")
        return out, gz, info

    def vfe_nuts_batch(self, X, Y, Z, q0, seeds, *a, **kw):
        self.seeds_seen = [int(s) for s in seeds]
        return super().vfe_nuts_batch(X, Y, Z, q0, seeds, *a, **kw)


def test_start_redraw_and_the_user_start():
    X, Y, Z = toy(B=3)
    base = np.array([math.log(2.0), 0.0, 0.0])
    eng = ZeroDensityAtFirst(who=1, rounds=2)
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 3, 3, seed=4, engine=eng)
    assert eng.value_only == 3 and (r.info == 0).all()   # two rounds with a bad chain, the third finds none
    for b in range(3):  # hmc._find_start: test point + U(-1, 1) from the chain's own SplitMix, redrawn for the chain that failed alone
        s = SplitMix(ggp_amd.chain_seed(4, b, 0))
        draws = [base + s.uniform(-1.0, 1.0, 3) for _ in range(3 if b == 1 else 1)]
        assert np.array_equal(r.starts[b, 0], draws[-1]) and eng.seeds_seen[b] == s.s   # the sampler continues that stream
    never = ZeroDensityAtFirst(who=0, rounds=10 ** 6)   # the density never becomes finite: 1 + 20 draws, then the chain is left to report
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y[:1], Z, 3, 3, seed=4, engine=never)
    assert never.value_only == 20 and (r.info == 0).all()
    # a user-supplied start is never replaced, never pre-checked
    eng = ZeroDensityAtFirst(who=1, rounds=5)
    q = np.array([0.3, 0.2, -0.4])
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 3, 3, seed=4, start=q, engine=eng)
    assert eng.value_only == 0 and (r.starts == q).all() and eng.seeds_seen == [ggp_amd.chain_seed(4, b, 0) for b in range(3)]
    per = np.stack([q + 0.1 * b for b in range(3)])[:, None, :]
    r2 = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 3, 3, seed=4, start=per, engine=VfeNutsDouble())
    assert np.array_equal(r2.starts, per) and np.array_equal(r2.samples[0], r.samples[0]) and not np.array_equal(r2.samples[1], r.samples[1])


def test_info_of_a_bad_start():
    X, Y, Z = toy(B=3)
    start = np.tile(np.array([0.3, 0.2, -0.4]), (3, 2, 1))
    start[0, 1, 0] = float("nan")
    start[2, 0, 2] = 300.0
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 4, 4, chains=2, seed=9, start=start, engine=VfeNutsDouble())
    bad = np.zeros((3, 2), dtype=bool)
    bad[0, 1] = bad[2, 0] = True
    assert np.array_equal(r.info, np.where(bad, L.VFE_NUTS_BAD_START, 0))
    assert np.isnan(r.samples[bad]).all() and np.isnan(r.stats[bad]).all() and np.isnan(r.seconds[bad]).all()
    assert np.isfinite(r.samples[~bad]).all() and (r.draws[bad] == 0).all() and (r.draws[~bad] == 8).all()
    good = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 4, 4, chains=2, seed=9, start=np.array([0.3, 0.2, -0.4]), engine=VfeNutsDouble())
    assert np.array_equal(good.samples[~bad], r.samples[~bad])
    assert np.isfinite(r.posterior_mean()).all()


def _fit_toy(engine, B=3):
    rng = np.random.default_rng(2)
    X = rng.uniform(-2.0, 2.0, (B, 20, 2))
    Y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, 20))
    return X, Y, ggp_amd.fit_sgpr_batch(X, Y, X[:, :5].copy(), max_steps=4, lr=0.05, seed=0, engine=engine)


def test_sgpr_batch_result_sample_nuts_on_a_toy_fit():
    eng = VfeNutsDouble()
    X, Y, fit = _fit_toy(eng)
    post = fit.sample_nuts(4, 5, chains=2, seed=6, max_treedepth=5)
    assert eng.calls["vfe_nuts_batch"] == 1 and post.samples.shape == (3, 2, 4, 4) and (post.info == 0).all() and (post.draws == 9).all()
    want = np.concatenate([np.log(fit.theta[:, :2]), 0.5 * np.log(fit.theta[:, 2:])], 1)   # the log of the fitted [ls | sig_f | sig_n]
    assert np.array_equal(post.starts, np.broadcast_to(want[:, None, :], (3, 2, 4)))
    assert np.array_equal(post.Z, fit.Z) and np.array_equal(post.X, X) and post.kernel == fit.kernel and post.jitter == fit.jitter
    assert np.array_equal(post.seeds, [[ggp_amd.chain_seed(6, b, c) for c in range(2)] for b in range(3)])
    assert (post.stats[..., 2] <= 5).all()   # the options reach the sampler
    again = ggp_amd.sample_sgpr_nuts_batch(X[1], Y[1], fit.Z[1], 4, 5, seeds=[[int(post.seeds[1, 1])]], start=want[1], max_treedepth=5,
                                           engine=VfeNutsDouble())
    assert np.array_equal(again.samples[0, 0], post.samples[1, 1])
    bare = ggp_amd.SgprBatchResult(**{**fit.__dict__, "X": None})
    with pytest.raises(ValueError, match="does not carry the data"):
        bare.sample_nuts(2, 2)


def test_model_feeds_the_mixture_predictive():
    from fake_engine import OracleEngine

    class Both(OracleEngine, VfeNutsDouble):
        def __init__(self):
            OracleEngine.__init__(self)
            self.fail, self.evaluator = None, self
            self.calls.update(vfe_eval_batch=0, vfe_nuts_batch=0)

    X, Y, Z = toy(B=2, N=14)
    r = ggp_amd.sample_sgpr_nuts_batch(X, Y, np.stack([Z, Z + 0.1]), 5, 6, seed=2, engine=Both())
    m = r.model(1)
    assert isinstance(m, ggp_amd.BayesianSparseGPR_HMC) and np.array_equal(m.inducing_points.numpy(), Z + 0.1)
    assert np.array_equal(m.train_x.numpy(), X) and np.array_equal(m.train_y.numpy(), Y[1]) and m.jitter == 1e-6
    Xt = T(np.linspace(-2.5, 2.5, 7)[:, None])
    preds = ggp_amd.mixture_posterior_predictive(m, Xt, r.traces[1][0])
    assert 1 <= len(preds) <= 5
    for p in preds:
        assert p.mean.shape == (7,) and torch.isfinite(p.mean).all() and torch.isfinite(p.variance).all() and (p.variance > 0).all()
    with pytest.raises(ValueError, match="RBF"):
        ggp_amd.SgprNutsResult(**{**r.__dict__, "kernel": "matern32"}).model(0)
    with pytest.raises(ValueError, match="does not carry the data"):
        ggp_amd.SgprNutsResult(**{**r.__dict__, "Z": None}).model(0)


def test_experiment_sparse_hmc_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from exact_nuts_double import ExactNutsDouble

    class Both(ExactNutsDouble, VfeNutsDouble):
        def __init__(self):
            ExactNutsDouble.__init__(self)
            self.fail = None
            self.calls.update(vfe_eval_batch=0, vfe_nuts_batch=0)

    base = ["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4", "--sparse", "4", "--sparse_steps", "3"]
    eng = Both()
    s = mod.main(base + ["--hmc", "--hmc_chains", "2", "--hmc_tune", "6", "--hmc_draws", "5", "--out", str(tmp_path / "both")], engine=eng)
    assert eng.calls["vfe_nuts_batch"] == 2 == eng.calls["exact_nuts_batch"]   # one batch per cell: the size cell and the noise cell
    z = np.load(tmp_path / "both" / "hyperparameter_identification.npz")
    for c in ("size", "noise"):
        for k in ("ls", "sf", "sn"):
            v = z["%s_sparse_hmc_%s" % (c, k)]
            assert v.shape == (1, 2) == z["%s_sparse_%s" % (c, k)].shape and np.isfinite(v).all() and (v > 0).all()
        assert z["%s_sparse_hmc_seconds" % c].shape == (1,) and 0.0 <= s["%s_sparse_hmc_diverging" % c][0] <= 1.0
        assert s["%s_sparse_hmc_seconds" % c] == z["%s_sparse_hmc_seconds" % c].tolist()
    assert "size_sparse_hmc_mean_log_ls" in json.load(open(tmp_path / "both" / "hyperparameter_identification.json"))
    # --sparse alone, and --hmc alone, record nothing of it
    for flags in ([], ["--hmc", "--hmc_chains", "1", "--hmc_tune", "3", "--hmc_draws", "3"]):
        eng = Both()
        args = (base if not flags else base[:8]) + flags
        s0 = mod.main(args + ["--out", str(tmp_path / ("plain%d" % len(flags)))], engine=eng)
        assert eng.calls["vfe_nuts_batch"] == 0 and not any("sparse_hmc" in k for k in s0)


# ---------------------------------------------------------------------------------------------------------------- the posterior pin
PIN_SEED = 1


def pin_run(engine):
    """8 chains x (400 tune + 150 draws) on the d = 1 fixture (N = 64, M = 8, jitter 1e-6), pooled: (draws x 3, share of diverging draws)."""
    P = load_golden("posterior_rbf_d1_tiny")
    r = ggp_amd.sample_sgpr_nuts_batch(P["X"], P["y"], P["Z"], 150, 400, chains=8, seed=PIN_SEED, jitter=float(P["jitter"]), engine=engine)
    assert (r.info == 0).all() and (r.draws == 550).all()
    return r.samples.reshape(-1, 3), float(r.stats[..., 4].mean())


def test_quadrature_posterior_pin_on_the_double():
    from test_posterior_pin import check_moments
    th, diverging = pin_run(VfeNutsDouble())
    assert diverging <= 0.01
    check_moments(th, load_golden("posterior_rbf_d1_tiny"), "sample_sgpr_nuts_batch / double")
