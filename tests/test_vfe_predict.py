"""CPU: the batched sparse-GP predictive around its kernel -- the ABI of libsgp_vfe_predict_hip.so, the host-side refusals, the
long-double reference's own checks (tests/vfe_predict_reference.py: the caps on its tolerance, deliberate defects, the two float64
orders), the CPU double (tests/vfe_predict_double.py) against it, ``predict_sgpr_batch`` / ``SgprNutsResult.predict`` /
``SgprBatchResult.predict`` and the experiment's ``--sparse M --holdout K [--hmc]`` on that double, and the plain-C++ part of
csrc/sgp_vfe_predict.hpp as a stand-alone host program under AddressSanitizer + UBSan.

The ``check_*`` functions are shared with tests/test_vfe_predict_gpu.py, which runs them on the device."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import vfe_batch_double as VB
import vfe_predict_reference as R
import vfe_reference as V
from conftest import ROOT
from exact_predict_reference import assert_mixture_close, mixture_reference
from test_vfe_batch_gpu import hetero_problem
from vfe_predict_double import VfePredictDouble

import ggp_amd
import ggp_amd._lib as L

CSRC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
NAMES = {"sgp_vfe_predict_batch_workspace_bytes": 5, "sgp_vfe_predict_batch_occupancy": 2, "sgp_vfe_predict_batch": 31,
         "sgp_ctx_vfe_predict_batch": 32}
ENTRY = ("libsgp_vfe_predict_hip.so", ["sgp_vfe_predict.hip"], "sgp_vfe_predict.h")
T_EDGE_CELLS = ["257-16-2-rbf", "17-31-2-rbf", "200-64-2-matern32"]   # one per size class
_host = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))  # noqa: E731  (a copy: the cells' arrays are read-only)


def np64(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(np64(a)), np.ascontiguousarray(np64(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- shared checks
def predict_cell(engine, conv, name, pred_noise=True, T=None, want_bound=True):
    inp = VB.inputs(name)
    Xs = R.cell_points(name) if T is None else R.cell_points(name, T)
    return engine.vfe_predict_batch(conv(inp["X"]), conv(inp["y"]), conv(inp["Z"]), conv(inp["theta"][None]), conv(Xs), kernel=inp["kernel"],
                                    jitter=inp["jitter"], pred_noise=pred_noise, want_bound=want_bound)


def check_cell(engine, conv, name):
    """Family (a) at one cell on ``engine`` (``conv``: numpy -> the engine's tensors): both ``pred_noise`` values against the long-double
    reference under the cell's own tolerance.  Returns the worst ratios to the tolerance."""
    inp = VB.inputs(name)
    sf2, s2 = float(inp["theta"][-2]), float(inp["theta"][-1])
    worst = {k: 0.0 for k in R.KEYS}
    for pred_noise in (False, True):
        mean, var, bound, info = predict_cell(engine, conv, name, pred_noise)
        T = R.cell_points(name).shape[0]
        assert int(info.item()) == 0 and tuple(mean.shape) == tuple(var.shape) == (1, T) and tuple(bound.shape) == (1,)
        got = {"mean": np64(mean)[0], "var": np64(var)[0]}
        w = R.assert_close(got, name, pred_noise, "noise=%d" % pred_noise)
        tol = R.tolerances(name, pred_noise)
        print("VFE_PREDICT %s noise=%d  mean %.2g of tol %.1e, var %.2g of tol %.1e" % (name, pred_noise, w["mean"], tol["mean"], w["var"],
                                                                                    tol["var"]))
        # the far point 100 * 1: k_u* underflows (to zero for the RBF), so the mean vanishes and the variance is the prior's
        assert abs(got["mean"][3]) <= 1e-80 and got["var"][3] == sf2 + (s2 if pred_noise else 0.0)
        if inp["kernel"] == "rbf":
            assert got["mean"][3] == 0.0
        worst = {k: max(worst[k], w[k]) for k in R.KEYS}
    return worst


def t_edges(name):
    tn = R.tile_rows(VB.spec(name)["M"])
    return [1, tn - 1, tn, tn + 1, 2 * tn + 1]


def check_t_edges(engine, conv, name, bits):
    """Family (b): T across the tile of the cell's class.  Each call meets the bound; with ``bits`` its points have the bits of the
    longest call's leading points."""
    Ts = t_edges(name)
    full = None
    for T in reversed(Ts):
        mean, var, _, info = predict_cell(engine, conv, name, True, T=T)
        assert int(info.item()) == 0 and tuple(mean.shape) == (1, T)
        R.assert_close({"mean": np64(mean)[0], "var": np64(var)[0]}, name, True, "T=%d" % T, T=Ts[-1], rows=T)
        if T == Ts[-1]:
            full = (mean, var)
        elif bits:
            assert same_bits(mean, full[0][:, :T]) and same_bits(var, full[1][:, :T]), T


def hetero_predict_problem(seed=5):
    """``test_vfe_batch_gpu.hetero_problem`` (P = 37 over 3 data sets x 2 targets x 3 inducing sets at (65, 17, 2)) plus two test sets of
    T = 70 points (two tiles of the middle class) and a test-set index per problem."""
    X, Y, Z, theta, ix, iy, iz = hetero_problem(seed)
    rng = np.random.default_rng(seed + 100)
    Xs = 1.5 * rng.standard_normal((2, 70, X.shape[2]))
    Xs[0, :5], Xs[1, :5] = X[0, :5], Z[1, :5]
    return X, Y, Z, theta, Xs, ix, iy, iz, rng.integers(0, 2, theta.shape[0])


def check_bound_is_the_batched_bound(engine, conv, kernel="matern52"):
    """Family (c): ``bound`` has the bits of ``vfe_eval_batch(want_grad=False)``'s F over a heterogeneous batch, ``info`` is equal, and
    ``want_bound=False`` changes no bit of mean / var."""
    X, Y, Z, theta, Xs, ix, iy, iz, ixs = hetero_predict_problem()
    Xd, Yd, Zd, thd, Xsd = (conv(a) for a in (X, Y, Z, theta, Xs))
    mean, var, bound, info = engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, ix=ix, iy=iy, iz=iz, ixs=ixs, kernel=kernel, jitter=1e-6)
    out, _, info_b = engine.vfe_eval_batch(Xd, Yd, Zd, thd, ix=ix, iy=iy, iz=iz, kernel=kernel, jitter=1e-6, want_grad=False)
    assert np.array_equal(np64(info), np64(info_b)) and int(np.abs(np64(info)).sum()) == 0
    assert same_bits(bound, out[:, 0].contiguous()) and np.isfinite(np64(bound)).all()
    m2, v2, none, i2 = engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, ix=ix, iy=iy, iz=iz, ixs=ixs, kernel=kernel, jitter=1e-6,
                                                want_bound=False)
    assert none is None and same_bits(m2, mean) and same_bits(v2, var) and np.array_equal(np64(i2), np64(info))
    d = X.shape[2]
    for p in (0, 7, 19, 30, 36):   # against the reference: these well-conditioned problems lie at the FLOOR of the tolerance rule
        args = (X[ix[p]], Y[iy[p]], Z[iz[p]], Xs[ixs[p]], theta[p, :d], theta[p, d], theta[p, d + 1], 1e-6, kernel)
        ref, S = R.predictive(*args)
        e = {k: 0.0 for k in R.KEYS}
        for order in ("inverse", "substitution"):
            w = R.worst(R.predictive(*args, True, np.float64, order)[0], ref, S)
            e = {k: max(e[k], w[k]) for k in R.KEYS}
        w = R.worst({"mean": np64(mean)[p], "var": np64(var)[p]}, ref, S)
        assert all(w[k] <= V.tolerance(e[k]) for k in R.KEYS), (p, w, e)
    return mean, var, bound, info


def check_failures_stay_local(engine, conv):
    """Family (e): a theta row with a NaN, a zero or a negative entry, and a K that fails (duplicate Z with J = 0): NaN rows, the right
    ``info``, bit-identical neighbours."""
    X, Y, Z, theta, Xs, ix, iy, iz, ixs = hetero_predict_problem(seed=6)
    P, d, M = 8, 2, 17
    theta, ix, iy, iz, ixs = theta[:P].copy(), ix[:P], iy[:P], iz[:P].copy(), ixs[:P]
    Zdup = Z[0].copy()
    Zdup[1] = Zdup[0]
    Xd, Yd, Zd, Xsd = conv(X), conv(Y), conv(np.concatenate([Z, Zdup[None]])), conv(Xs)
    call = lambda th, iz_: engine.vfe_predict_batch(Xd, Yd, Zd, conv(th), Xsd, ix=ix, iy=iy, iz=iz_, ixs=ixs, kernel="rbf", jitter=0.0)  # noqa: E731
    gm, gv, gb, gi = call(theta, iz)
    assert int(np.abs(np64(gi)).sum()) == 0 and np.isfinite(np64(gm)).all() and np.isfinite(np64(gv)).all()
    cases = {"nan": (1, 0, np.nan), "zero": (2, d, 0.0), "negative": (4, d + 1, -0.3), "inf": (6, 1, np.inf)}
    for what, (p, col, value) in cases.items():
        th = theta.copy()
        th[p, col] = value
        m, v, b, i = call(th, iz)
        keep = [q for q in range(P) if q != p]
        assert np64(i).tolist() == [1 if q == p else 0 for q in range(P)], what
        assert np.isnan(np64(m)[p]).all() and np.isnan(np64(v)[p]).all() and np.isnan(np64(b)[p]), what
        assert same_bits(m[keep], gm[keep]) and same_bits(v[keep], gv[keep]) and same_bits(b[keep], gb[keep]), what
    izd = iz.copy()
    izd[3] = 3
    m, v, b, i = call(theta, izd)
    keep = [q for q in range(P) if q != 3]
    assert 1 <= int(np64(i)[3]) <= M and np64(i)[keep].tolist() == [0] * (P - 1)
    assert np.isnan(np64(m)[3]).all() and np.isnan(np64(v)[3]).all() and np.isnan(np64(b)[3])
    assert same_bits(m[keep], gm[keep]) and same_bits(v[keep], gv[keep]) and same_bits(b[keep], gb[keep])


def check_mixture_of_draws(r, Y_test):
    """The mixture fields of a ``SgprMixturePredictive`` against the long-double mixture of its own ``draw_mean`` / ``draw_var`` under
    ``mixture_reference``'s derived bounds."""
    worst = {}
    for b in range(r.mean.shape[0]):
        ref = mixture_reference(r.draw_mean[b], r.draw_var[b], r.info[b], None if Y_test is None else Y_test[b])
        assert ref["kept"] == r.kept[b]
        keys = ("mean", "var") + (() if Y_test is None else ("logpdf", "mean_logpdf"))
        w = assert_mixture_close({k: getattr(r, k)[b] for k in keys}, ref, "data set %d" % b)
        worst.update({k: max(worst.get(k, 0.0), w[k]) for k in w})
    return worst


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load_vfe_predict_library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    """The companion library libsgp_vfe_predict_hip.so: include/sgp_vfe_predict.h = its dynamic symbol table = VFE_PREDICT_PROTOTYPES,
    and neither the core library's surface (include/sgp.h) nor another companion's table has any of it."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp_vfe_predict.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sgp_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(L.VFE_PREDICT_PROTOTYPES)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.VFE_PREDICT_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", L.VFE_PREDICT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(NAMES)
    und = subprocess.run([nm, "-D", "--undefined-only", L.VFE_PREDICT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert [ln.split()[-1] for ln in und.splitlines() if re.search(r"\bsgp_", ln)] == ["sgp_ctx_device"]   # all it takes from the core
    core = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert "sgp_vfe_predict" not in core and L.SGP_ABI_VERSION == 3 and len(L.PROTOTYPES) == 146
    for table in (L.PROTOTYPES, L.EXACT_NUTS_PROTOTYPES, L.EXACT_PREDICT_PROTOTYPES, L.VFE_BATCH_PROTOTYPES, L.VFE_NUTS_PROTOTYPES):
        assert not any(n in table for n in NAMES)
    assert L._COMPANION_TABLE["vfe_predict"] == (L.VFE_PREDICT_LIB_PATH, L.VFE_PREDICT_PROTOTYPES) and L.VFE_PREDICT_MAX_T == 32768
    assert hasattr(ggp_amd.HipEngine, "vfe_predict_batch") and hasattr(ggp_amd.HipEngine, "vfe_predict_lib")
    import ggp_amd.build as B
    assert B.COMPANIONS.count(ENTRY) == 1
    assert [c[1] for c in B.COMPANIONS].count(["sgp_vfe_predict.hip"]) == 1 and "sgp_vfe_predict.hip" not in B.SOURCES


def test_the_digest_covers_the_new_library(lib, tmp_path, monkeypatch):
    """build() reuses the library while its digest is unchanged: its source, its header and every csrc header it includes are in it."""
    spec = importlib.util.spec_from_file_location("_sgp_build_vp", os.path.join(ROOT, "generalised-gaussian-processes_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    (name, sources, header), = [c for c in b.COMPANIONS if c[0] == "libsgp_vfe_predict_hip.so"]
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
    for edited in (work / "sgp_vfe_predict.hip", work / "sgp_vfe_predict.hpp", work / "sgp_vfe_batch.hpp", work / "sgp_wg_dense.hpp",
                   work / "sgp_common.hpp", tmp_path / "include" / header):
        with open(edited, "a") as fh:
            fh.write("// a comment\n")
        after = b._companion_digest(b._digest(), sources, header)
        assert after != before, edited
        before = after


# ---------------------------------------------------------------------------------------------------------------- refusals, no device
def _args(**bad):
    a = dict(X=8, Y=8, Z=8, Xs=8, th=8, out=8, P=4, N=10, M=5, d=2, T=7, ldx=2, ldz=2, ldxs=2, kid=0, jitter=1e-6, ws=8, nbytes=256,
             bound=8, stride=20)
    a.update(bad)
    p = lambda k: C.c_void_p(a[k])  # noqa: E731  (the dummy 8 is never dereferenced: every call here fails validation first)
    return (p("X"), a["stride"], a["ldx"], p("Y"), a["N"], None, None, p("Z"), a["M"] * a["d"], a["ldz"], None, p("Xs"), a["T"] * a["d"],
            a["ldxs"], a["T"], None, p("th"), a["P"], a["N"], a["M"], a["d"], a["kid"], a["jitter"], 1, p("out"), p("out"), p("bound"),
            p("out"), p("ws"), a["nbytes"], None)


ROWS = [  # (what is wrong, status): SGP_ERR_ARG = -1 before SGP_ERR_DIM = -2 before SGP_ERR_WORKSPACE = -3, all before any launch
    (dict(M=65), -2), (dict(N=65537), -2), (dict(d=9, ldx=9, ldz=9, ldxs=9), -2), (dict(P=2 ** 24), -2), (dict(T=32769), -2),
    (dict(kid=3), -1), (dict(kid=-1), -1), (dict(P=0), -1), (dict(N=0), -1), (dict(M=0), -1), (dict(d=0), -1), (dict(T=0), -1),
    (dict(X=0), -1), (dict(Y=0), -1), (dict(Z=0), -1), (dict(Xs=0), -1), (dict(th=0), -1), (dict(out=0), -1), (dict(ldx=1), -1),
    (dict(ldz=1), -1), (dict(ldxs=1), -1), (dict(stride=-1), -1), (dict(jitter=-1e-6), -1), (dict(jitter=float("nan")), -1),
    (dict(ws=0), -3), (dict(nbytes=255), -3), (dict(N=3, M=5, nbytes=255), -3),   # M > N is legal: it gets as far as the workspace
    (dict(M=65, kid=3), -1), (dict(M=65, out=0), -1), (dict(T=32769, Xs=0), -1), (dict(T=32769, P=0), -1),
    (dict(M=65, ws=0), -2), (dict(T=32769, nbytes=0), -2), (dict(jitter=-1.0, ws=0), -1),
]


def test_out_of_range_arguments_are_refused_on_the_host(lib):
    for bad, want in ROWS:
        assert lib.sgp_vfe_predict_batch(*_args(**bad)) == want, bad
        assert lib.sgp_ctx_vfe_predict_batch(None, *_args(**bad)) == want, bad
    q = lib.sgp_vfe_predict_batch_workspace_bytes
    assert q(1, 1, 1, 1, 1) == 256 == q(2 ** 24 - 1, 65536, 64, 8, 32768) and q(2, 3, 5, 1, 9) == 256
    for shape in [(4, 10, 65, 1, 5), (4, 65537, 5, 1, 5), (4, 10, 5, 9, 5), (0, 10, 5, 1, 5), (2 ** 24, 10, 5, 2, 5), (4, 0, 5, 1, 5),
                  (4, 10, 0, 1, 5), (4, 10, 5, 0, 5), (4, 10, 5, 1, 0), (4, 10, 5, 1, 32769)]:
        assert q(*shape) == 0, shape
    occ = lib.sgp_vfe_predict_batch_occupancy
    assert occ(65, 0) == -2 and occ(10, 3) == -1 and occ(0, 0) == -1 and occ(65, 3) == -1


# ---------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name", R.CELLS)
def test_the_tolerance_rule_cannot_hide_a_failure(name):
    """tol = 10 max(e64, 1e-13) stays at or below 1e-10 at every untagged cell and 1e-8 at the three tagged ones, for both outputs and
    both ``pred_noise`` values; the two float64 orders themselves lie within it (by a factor 10), and the double does."""
    cap = R.CAP_TAGGED if name in R.TAGGED else R.CAP_UNTAGGED
    for pred_noise in (True, False):
        tol = R.tolerances(name, pred_noise)
        assert all(1e-12 <= tol[k] <= cap for k in R.KEYS), (name, pred_noise, tol)
        ref, S = R.reference(name, pred_noise)
        for order in ("inverse", "substitution"):
            w = R.worst(R.evaluate(name, pred_noise, np.float64, order)[0], ref, S)
            assert all(w[k] <= tol[k] / 10 * (1 + 1e-12) for k in R.KEYS), (order, w, tol)
    check_cell(VfePredictDouble(), _host, name)


@pytest.mark.parametrize("name", R.CELLS)
def test_deliberate_defects_fail_the_comparison(name):
    ref, S = R.reference(name, True)
    tol = R.tolerances(name, True)
    assert R.MUTATIONS == ("no_v2", "no_jitter", "no_noise")
    for mutate, least in (("no_v2", 4.7e-4), ("no_jitter", 3.6e-7), ("no_noise", 1e-4)):
        try:
            bad = R.evaluate(name, True, mutate=mutate)[0]
        except np.linalg.LinAlgError:
            assert mutate == "no_jitter" and name == "200-64-2-rbf-ill"   # its K_uu does not factor without the jitter, even in long double
            continue
        w = R.worst(bad, ref, S)
        assert w["var"] > tol["var"] and w["var"] >= least * 0.5, (mutate, w, tol)
        assert w["mean"] <= tol["mean"] or mutate == "no_jitter"   # (the other two touch the variance alone)
        with pytest.raises(AssertionError):
            R.assert_close(bad, name, True)
    # pred_noise = False ignores the noise already: the defect is invisible there, which is why both values are tested
    assert R.worst(R.evaluate(name, False, mutate="no_noise")[0], *R.reference(name, False))["var"] == 0.0


@pytest.mark.parametrize("name", T_EDGE_CELLS)
def test_the_double_meets_the_bound_at_the_t_edges(name):
    check_t_edges(VfePredictDouble(), _host, name, bits=False)


def test_the_double_reports_the_bound_and_failures_like_the_kernel():
    eng = VfePredictDouble()
    check_bound_is_the_batched_bound(eng, _host)
    check_failures_stay_local(eng, _host)
    X, Y, Z, theta, Xs, ix, iy, iz, ixs = hetero_predict_problem()
    with pytest.raises(ValueError):
        eng.vfe_predict_batch(X, Y, Z, theta, Xs, ixs=[2] * 37)
    with pytest.raises(ValueError):
        eng.vfe_predict_batch(X, Y, np.zeros((65, 2)), theta, Xs[0])
    forced = VfePredictDouble(fail=lambda call, p: p == 2)
    m, v, b, i = forced.vfe_predict_batch(X[0], Y[0], Z[0], theta[:4], Xs[0])
    assert i.tolist() == [0, 0, 1, 0] and bool(m[2].isnan().all()) and bool(b[2].isnan()) and bool(m[[0, 1, 3]].isfinite().all())


# ---------------------------------------------------------------------------------------------------------------- the public layer
def _toy(B=3, N=14, d=2, M=5, S=4, T=6, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (B, N, d))
    Y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, N))
    Z = X[:, :M].copy() + 0.01
    Xt = rng.uniform(-2.0, 2.0, (B, T, d))
    Yt = np.sin(Xt.sum(2)) + 0.1 * rng.standard_normal((B, T))
    q = rng.uniform(-0.5, 0.5, (B, S, d + 2))
    q[..., -1] -= 1.5
    return X, Y, Z, Xt, Yt, q


def test_predict_sgpr_batch_shapes_and_the_mixture():
    X, Y, Z, Xt, Yt, q = _toy()
    B, S, T = q.shape[0], q.shape[1], Xt.shape[1]
    eng = VfePredictDouble()
    r = ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, Yt, kernel="matern32", engine=eng)
    assert isinstance(r, ggp_amd.SgprMixturePredictive) and isinstance(r, ggp_amd.ExactMixturePredictive)
    assert eng.calls["vfe_predict_batch"] == 1 and eng.calls["exact_mixture"] == 1
    assert r.mean.shape == r.var.shape == r.logpdf.shape == r.mean_logpdf.shape == (B, T)
    assert r.draw_mean.shape == r.draw_var.shape == (B, S, T) and r.info.shape == r.bound.shape == (B, S) and r.kept.tolist() == [S] * B
    assert np.isfinite(r.bound).all() and np.isfinite(r.nlpd()).all() and np.isfinite(r.rmse(Yt)).all()
    check_mixture_of_draws(r, Yt)
    # theta = [exp, exp^2, exp^2] with no floor and no jitter on the noise; the bound is vfe_eval_batch's at every draw
    th = np.concatenate([np.exp(q[..., :-2]), np.exp(q[..., -2:]) ** 2], -1)
    set_of = np.repeat(np.arange(B), S)
    m, v, b, _ = eng.vfe_predict_batch(X, Y, Z, th.reshape(B * S, -1), Xt, ix=set_of, iy=set_of, iz=set_of, ixs=set_of, kernel="matern32")
    assert np.array_equal(m.numpy().reshape(B, S, T), r.draw_mean) and np.array_equal(v.numpy().reshape(B, S, T), r.draw_var)
    out, _, _ = eng.vfe_eval_batch(X, Y, Z, th.reshape(B * S, -1), ix=set_of, iy=set_of, iz=set_of, kernel="matern32", want_grad=False)
    assert np.array_equal(out[:, 0].numpy().reshape(B, S), r.bound) and np.array_equal(b.numpy().reshape(B, S), r.bound)
    rt = ggp_amd.sgpr_predict.predict_sgpr_theta_batch(X, Y, Z, th, Xt, Yt, kernel="matern32", engine=eng)
    assert np.array_equal(rt.draw_var, r.draw_var) and np.array_equal(rt.logpdf, r.logpdf)
    # every data set alone, with X / Z / X_test given as 2-d arrays, is the same problem
    for bi in range(B):
        rb = ggp_amd.predict_sgpr_batch(X[bi], Y[bi], Z[bi], q[bi], Xt[bi], Yt[bi], kernel="matern32", engine=eng)
        assert np.array_equal(rb.draw_mean[0], r.draw_mean[bi]) and np.array_equal(rb.logpdf[0], r.logpdf[bi])
    shared = ggp_amd.predict_sgpr_batch(X[0], Y, Z[0], q, Xt[0], engine=eng)
    assert shared.mean.shape == (B, T) and shared.logpdf is None and shared.mean_logpdf is None
    with pytest.raises(ValueError):
        shared.nlpd()
    mixed = ggp_amd.predict_sgpr_batch(X[0], Y, Z, q, Xt, kernel="matern32", engine=eng)   # shared X, per-set Z and X_test
    assert np.array_equal(mixed.draw_mean[0], r.draw_mean[0]) and not np.array_equal(mixed.draw_mean[1], r.draw_mean[1])
    # the jitter goes on K_uu, not on the noise: it moves the predictive, and theta is untouched by it
    jit = ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, kernel="matern32", jitter=1e-2, engine=eng)
    m2, _, _, _ = eng.vfe_predict_batch(X[0], Y[0], Z[0], th[0], Xt[0], kernel="matern32", jitter=1e-2)
    assert np.array_equal(m2.numpy(), jit.draw_mean[0]) and not np.array_equal(jit.draw_mean, r.draw_mean)
    lat = ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, kernel="matern32", pred_noise=False, engine=eng)
    assert np.allclose(lat.draw_var + th[..., -1:], r.draw_var, rtol=1e-12) and np.array_equal(lat.draw_mean, r.draw_mean)


def test_no_noise_floor_nan_rows_and_shape_errors():
    X, Y, Z, Xt, Yt, q = _toy(B=2)
    q[0, 1, -1] = np.log(1e-3)    # sig_n^2 = 1e-6: the sparse route has no floor, the draw is predicted at s2 = 1e-6
    q[1, 2] = np.nan              # a chain that had no start
    before = q.copy()
    eng = VfePredictDouble()
    r = ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, Yt, engine=eng)
    assert np.array_equal(q, before, equal_nan=True)
    assert r.kept.tolist() == [4, 3] and r.info[1, 2] == 1 and r.info.sum() == 1
    assert np.isnan(r.draw_mean[1, 2]).all() and np.isnan(r.bound[1, 2]) and np.isfinite(np.delete(r.bound.reshape(-1), 6)).all()
    assert np.isfinite(r.mean).all() and np.isfinite(r.logpdf).all()
    assert np.allclose(r.mean[1], r.draw_mean[1, [0, 1, 3]].mean(0), rtol=1e-13)
    check_mixture_of_draws(r, Yt)
    th = np.concatenate([np.exp(q[0, 1, :2]), [np.exp(q[0, 1, 2]) ** 2, np.exp(q[0, 1, 3]) ** 2]])
    assert abs(th[-1] - 1e-6) < 1e-18
    _, v, _, _ = eng.vfe_predict_batch(X[0], Y[0], Z[0], th[None], Xt[0])
    assert np.array_equal(v.numpy()[0], r.draw_var[0, 1])
    for bad in (dict(Y_test=Yt[:, :3]), dict(Y_test=Yt[:1]), dict(Y_test=np.zeros(5))):
        with pytest.raises(ValueError, match="Y_test"):
            ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, engine=eng, **bad)
    with pytest.raises(ValueError, match="Z must be"):
        ggp_amd.predict_sgpr_batch(X, Y, np.zeros((3, 5, 2)), q, Xt, engine=eng)
    with pytest.raises(ValueError, match="Z must be"):
        ggp_amd.predict_sgpr_batch(X, Y, np.zeros((65, 2)), q, Xt, engine=eng)
    with pytest.raises(ValueError, match="X_test"):
        ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt[:, :, :1], engine=eng)
    with pytest.raises(ValueError, match="draws"):
        ggp_amd.predict_sgpr_batch(X, Y, Z, q[:, :, :3], Xt, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, kernel="composite", engine=eng)


def test_results_carry_what_predict_needs():
    rng = np.random.default_rng(5)
    B, N, M = 2, 12, 4
    X = np.sort(rng.uniform(-3.0, 3.0, (N, 1)), 0)
    Y = np.sin(X[:, 0])[None] + 0.2 * rng.standard_normal((B, N))
    Z = X[np.round(np.linspace(0, N - 1, M)).astype(int)].copy()
    Xt, Yt = rng.uniform(-3.0, 3.0, (6, 1)), rng.standard_normal((B, 6))
    eng = VfePredictDouble()
    post = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 6, 8, chains=2, seed=1, jitter=1e-5, engine=eng)
    r = post.predict(Xt, Yt, thin=2)
    assert isinstance(r, ggp_amd.SgprMixturePredictive) and r.draw_mean.shape == (B, 2 * 3, 6) and r.kept.tolist() == [6, 6]
    assert np.isfinite(r.nlpd()).all() and np.isfinite(r.rmse(Yt)).all()
    want = ggp_amd.predict_sgpr_batch(X, Y, Z, post.samples[:, :, ::2].reshape(B, 6, 3), Xt, Yt, jitter=1e-5, engine=eng)
    assert np.array_equal(want.draw_mean, r.draw_mean) and np.array_equal(want.logpdf, r.logpdf) and np.array_equal(want.bound, r.bound)
    other = ggp_amd.predict_sgpr_batch(X, Y, Z, post.samples[:, :, ::2].reshape(B, 6, 3), Xt, Yt, jitter=1e-3, engine=eng)
    assert not np.array_equal(other.draw_mean, r.draw_mean)   # the result's own jitter reached the kernel
    assert post.predict(Xt).draw_mean.shape == (B, 12, 6) and post.predict(Xt, pred_noise=False).var.shape == (B, 6)
    with pytest.raises(ValueError):
        post.predict(Xt, thin=0)
    for missing in ("X", "Y", "Z", "kernel"):
        with pytest.raises(ValueError, match="does not carry the data"):
            ggp_amd.SgprNutsResult(**{**post.__dict__, missing: None}).predict(Xt)
    # the plug-in predictive of a fit: S = 1 at the fitted theta and Z, no exp
    Xf = rng.uniform(-2.0, 2.0, (3, 20, 2))
    Yf = np.sin(Xf.sum(2)) + 0.1 * rng.standard_normal((3, 20))
    fit = ggp_amd.fit_sgpr_batch(Xf, Yf, Xf[:, :5].copy(), max_steps=3, lr=0.05, seed=0, engine=eng)
    Xg, Yg = rng.uniform(-2.0, 2.0, (3, 7, 2)), rng.standard_normal((3, 7))
    p = fit.predict(Xg, Yg)
    assert p.draw_mean.shape == (3, 1, 7) and p.kept.tolist() == [1, 1, 1] and np.isfinite(p.nlpd()).all() and np.isfinite(p.rmse(Yg)).all()
    assert np.array_equal(p.mean, p.draw_mean[:, 0]) and np.array_equal(p.var, p.draw_var[:, 0])
    m, _, b, _ = eng.vfe_predict_batch(Xf, Yf, fit.Z, fit.theta, Xg, ix=[0, 1, 2], iy=[0, 1, 2], iz=[0, 1, 2], ixs=[0, 1, 2],
                                       kernel=fit.kernel, jitter=fit.jitter)
    assert np.array_equal(m.numpy(), p.mean) and np.array_equal(b.numpy(), p.bound[:, 0])
    shared = ggp_amd.fit_sgpr_batch(Xf[0], Yf, Xf[0, :5].copy(), max_steps=2, lr=0.05, seed=0, engine=eng)   # one X for all data sets
    assert shared.predict(Xg[0]).mean.shape == (3, 7)
    with pytest.raises(ValueError, match="does not carry the data"):
        ggp_amd.SgprBatchResult(**{**fit.__dict__, "X": None}).predict(Xg)


def test_experiment_sparse_holdout_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4", "--sparse", "4", "--sparse_steps", "3"]
    hmc = ["--hmc", "--hmc_chains", "2", "--hmc_tune", "6", "--hmc_draws", "5"]
    eng = VfePredictDouble()
    s = mod.main(base + hmc + ["--holdout", "5", "--out", str(tmp_path / "held")], engine=eng)
    new = ["%s_%s_%s" % (c, m, k) for c in ("size", "noise") for m in ("sparse", "sparse_hmc") for k in ("nlpd", "rmse")]
    old = ["%s_%s_%s" % (c, m, k) for c in ("size", "noise") for m in ("ml2", "hmc") for k in ("nlpd", "rmse")]
    for k in new + old:
        assert len(s[k]) == 1 and np.isfinite(s[k]).all(), k
    assert eng.calls["vfe_predict_batch"] == 4 == eng.calls["exact_predict_batch"]   # per cell: the plug-in and the mixture
    z = np.load(tmp_path / "held" / "hyperparameter_identification.npz")
    for c in ("size", "noise"):
        for m in ("sparse", "sparse_hmc"):
            assert z["%s_%s_nlpd" % (c, m)].shape == z["%s_%s_rmse" % (c, m)].shape == (1, 2)
    assert set(new) <= set(json.load(open(tmp_path / "held" / "hyperparameter_identification.json")))
    # --sparse --holdout without --hmc: the plug-in alone
    eng1 = VfePredictDouble()
    s1 = mod.main(base + ["--holdout", "5", "--out", str(tmp_path / "plug")], engine=eng1)
    assert eng1.calls["vfe_predict_batch"] == 2 and "size_sparse_nlpd" in s1 and not any("sparse_hmc" in k for k in s1)
    # without --holdout, and without --sparse, a run writes what it wrote before: the sparse predictive is never called
    eng0 = VfePredictDouble()
    s0 = mod.main(base + hmc + ["--out", str(tmp_path / "plain")], engine=eng0)
    assert set(s0) == set(s) - set(new) - set(old) and eng0.calls["vfe_predict_batch"] == 0
    z0 = np.load(tmp_path / "plain" / "hyperparameter_identification.npz")
    assert set(z0.files) == {k for k in z.files if not k.endswith(("_nlpd", "_rmse"))}
    eng2 = VfePredictDouble()
    s2 = mod.main(base[:8] + hmc + ["--holdout", "5", "--out", str(tmp_path / "exact")], engine=eng2)
    assert set(s2) == {k for k in s if "sparse" not in k} and eng2.calls["vfe_predict_batch"] == 0


# ---------------------------------------------------------------------------------------------------------------- the host program
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_host_part_of_the_header_under_asan_ubsan(tmp_path):
    """tests/native/vfe_predict_host.cpp (its own main) over the plain-C++ part of csrc/sgp_vfe_predict.hpp: the shape check with the
    order of its refusals, and the workspace query.  Built by g++ alone and run directly."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on CPU-only hosts, never on a GPU box")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "vfe_predict_host_asan")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-I", CSRC, "-o", exe,
                                                                           os.path.join(ROOT, "tests", "native", "vfe_predict_host.cpp")],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "vfe predict host ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
