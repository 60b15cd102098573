"""CPU: the batched exact-GP predictive around its kernels -- the ABI of libsgp_exact_predict_hip.so, the host-side refusals, the CPU
double (tests/exact_predict_double.py) against the long-double reference at the cells the GPU tests use, ``predict_exact_batch`` /
``ExactNutsResult.predict`` / ``Ml2Result.predict`` and the experiment's ``--holdout`` on that double, and the mixture's per-point
arithmetic (csrc/sgp_exact_predict.hpp) as a stand-alone host program under AddressSanitizer + UBSan."""
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

from conftest import ROOT
from exact_predict_double import ExactPredictDouble
from exact_predict_reference import TAU, assert_mixture_close, mixture_reference, ratios, reference
from test_exact_batch_gpu import DS, KS, NS, spread_theta

import ggp_amd
import ggp_amd._lib as L
from ggp_amd import metrics

CSRC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
NAMES = {"sgp_exact_predict_batch_workspace_bytes": 4, "sgp_exact_predict_batch_occupancy": 2, "sgp_exact_predict_batch": 24,
         "sgp_ctx_exact_predict_batch": 25, "sgp_exact_mixture_workspace_bytes": 2, "sgp_exact_mixture_reduce": 15}
# (a): one (d, kernel) per N, both rotated -- every d and every kernel meets the small (N <= 32), the middle and the large class
CELLS_A = [(N, DS[i % 3], KS[(i + 1) % 3]) for i, N in enumerate(NS)]
# (b): T across the 16-point tile, at a small and at the largest problem
CELLS_B = [(17, 1), (128, 8)]
TS = [1, 15, 16, 17, 33, 100]
_host = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)  # noqa: E731


def edge_problem(N, d, kernel):
    """X, y as test_exact_batch_gpu's edge-shape test draws them, its seven theta rows, and the test points: 20 uniform in [0, 10]^d,
    the first min(N, 8) training rows, training row 0 + 1e-9, and one point at 100."""
    rng = np.random.default_rng(1000 * N + d)
    X = rng.uniform(0.0, 10.0, (N, d))
    y = 3.0 * rng.standard_normal(N)
    Xs = np.concatenate([rng.uniform(0.0, 10.0, (20, d)), X[:min(N, 8)], X[:1] + 1e-9, np.full((1, d), 100.0)])
    return X, y, Xs, spread_theta(X, kernel)


def check_edge_cell(engine, conv, N, d, kernel):
    """Family (a) at one cell on ``engine`` (``conv``: numpy -> the engine's tensors).  Returns the worst ratios to the bound."""
    X, y, Xs, th = edge_problem(N, d, kernel)
    refs = [reference(X, y, Xs, th[p, :d], th[p, d], th[p, d + 1], kernel, pred_noise=False) for p in range(th.shape[0])]
    conds = [r["cond"] for r in refs]
    worst = [0.0, 0.0]
    for pred_noise in (False, True):
        mean, var, info = engine.exact_predict_batch(conv(X), conv(y), conv(th), conv(Xs), kernel=kernel, pred_noise=pred_noise)
        assert int(info.abs().sum()) == 0 and tuple(mean.shape) == tuple(var.shape) == (th.shape[0], Xs.shape[0])
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        for p, ref in enumerate(refs):
            ref = dict(ref, var=ref["var"] + np.longdouble(th[p, d + 1])) if pred_noise else ref
            rm, rv = ratios(mean[p], var[p], ref)
            print("N=%d d=%d %s noise=%d p=%d cond %.2e: |dmu|/S_mu %.2e, |dv|/S_v %.2e" % (N, d, kernel, pred_noise, p, ref["cond"], rm, rv))
            assert rm <= TAU and rv <= TAU, (p, ref["cond"], rm, rv)
            worst = [max(worst[0], rm), max(worst[1], rv)]
    if N > 1:
        assert min(conds) < 10.0 and 1e6 <= max(conds) <= 1e8, conds
    return worst


def t_edge_problem(N, d):
    """Family (b): 100 test points (the first 10 are training rows), three theta rows of spread_theta (cond 2, 3e3, 1e7)."""
    rng = np.random.default_rng(77 * N + d)
    X = rng.uniform(0.0, 10.0, (N, d))
    y = 3.0 * rng.standard_normal(N)
    Xs = np.concatenate([X[:min(N, 10)], rng.uniform(0.0, 10.0, (100 - min(N, 10), d))])
    return X, y, Xs, spread_theta(X, "rbf")[[0, 3, 6]]


def check_t_edges(engine, conv, N, d, same_bits):
    X, y, Xs, th = t_edge_problem(N, d)
    refs = [reference(X, y, Xs, th[p, :d], th[p, d], th[p, d + 1]) for p in range(3)]
    full = None
    for T in reversed(TS):
        mean, var, info = engine.exact_predict_batch(conv(X), conv(y), conv(th), conv(Xs[:T]))
        assert int(info.abs().sum()) == 0
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        for p, ref in enumerate(refs):
            cut = {k: (v[:T] if k in ("mean", "var", "S_mu", "S_v") else v) for k, v in ref.items()}
            rm, rv = ratios(mean[p], var[p], cut)
            assert rm <= TAU and rv <= TAU, (T, p, rm, rv)
        if T == 100:
            full = (mean, var)
        elif same_bits:
            assert np.array_equal(mean.view(np.uint64), full[0][:, :T].view(np.uint64)), T
            assert np.array_equal(var.view(np.uint64), full[1][:, :T].view(np.uint64)), T


def mixture_case(engine, conv):
    """Family (g): groups of 1, 2, 64 and 3 draws at T = 33, their moments from ``engine.exact_predict_batch``.  The last group's draws
    have all failed (non-positive theta): n = 0.  Ytest sits near the draws; one draw of the large group is moved to |y - mu| / sqrt(v) =
    50 (its density underflows beside the others), and in the group of two every draw has q = (y - mu)^2 / (2 v) ~ 1e4.
    Returns (mean, var, info, offsets, Ytest): engine tensors, the host offsets, Ytest as numpy."""
    rng = np.random.default_rng(9)
    N, d, T = 24, 2, 33
    sizes = [1, 2, 64, 3]
    off = np.concatenate([[0], np.cumsum(sizes)])
    P = int(off[-1])
    X = rng.uniform(0.0, 10.0, (N, d))
    y = 2.0 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 10.0, (T, d))
    th = np.exp(rng.uniform(-0.3, 0.6, (P, d + 2)))
    th[off[3]:, d] = -1.0
    mean, var, info = engine.exact_predict_batch(conv(X), conv(y), conv(th), conv(Xs))
    special = int(off[2]) + 5
    mean = mean.clone()
    mean[special] = mean[int(off[2])] + 50.0 * var[special].sqrt() + 0.3 * var[int(off[2])].sqrt()
    m, v = mean.cpu().numpy(), var.cpu().numpy()
    Y = np.stack([m[off[g]] + 0.3 * np.sqrt(v[off[g]]) for g in range(3)] + [np.zeros(T)])
    Y[1] = m[off[1]] + 141.4 * np.sqrt(v[off[1]])
    Y[2] = m[special] - 50.0 * np.sqrt(v[special])
    return mean, var, info, off.tolist(), Y


def check_mixture(engine, conv):
    """Family (g) on ``engine``: with and without Ytest, against long double from the moments the reduction read."""
    mean, var, info, off, Y = mixture_case(engine, conv)
    m, v, i = mean.cpu().numpy(), var.cpu().numpy(), info.cpu().numpy()
    assert i[:off[3]].tolist() == [0] * off[3] and (i[off[3]:] != 0).all()
    worst = {}
    for Yt in (Y, None):
        r = engine.exact_mixture(mean, var, info, off, Ytest=None if Yt is None else conv(Yt))
        assert r["kept"].cpu().tolist() == [1, 2, 64, 0]
        assert (r["logpdf"] is None and r["mean_logpdf"] is None) if Yt is None else r["logpdf"].shape == (4, 33)
        keys = ("mean", "var") + (() if Yt is None else ("logpdf", "mean_logpdf"))
        got = {k: r[k].cpu().numpy() for k in keys}
        for g in range(3):
            ref = mixture_reference(m[off[g]:off[g + 1]], v[off[g]:off[g + 1]], i[off[g]:off[g + 1]], None if Yt is None else Yt[g])
            w = assert_mixture_close({k: got[k][g] for k in keys}, ref, "group %d" % g)
            worst.update({k: max(worst.get(k, 0.0), w[k]) for k in w})
        assert all(np.isnan(got[k][3]).all() for k in keys)
        if Yt is not None:
            z = np.abs(Yt[2] - m[off[2] + 5]) / np.sqrt(v[off[2] + 5])
            assert np.allclose(z, 50.0, rtol=1e-12)   # its term exp(-1250) is 1e-540 times its neighbours'
            assert np.isfinite(got["logpdf"][1]).all() and (got["logpdf"][1] < -9e3).all() and (got["logpdf"][1] > -1.2e4).all()
    print("worst error / derived bound:", worst)
    return worst


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load_exact_predict_library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp_exact_predict.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sgp_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(L.EXACT_PREDICT_PROTOTYPES)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.EXACT_PREDICT_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", L.EXACT_PREDICT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(NAMES)
    core = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert not any(re.search(r"\b%s\b" % n, core) for n in NAMES) and not any(n in L.PROTOTYPES for n in NAMES) and L.SGP_ABI_VERSION == 3
    assert not any(n in L.EXACT_NUTS_PROTOTYPES for n in NAMES)
    assert hasattr(ggp_amd.HipEngine, "exact_predict_batch") and hasattr(ggp_amd.HipEngine, "exact_mixture")
    import ggp_amd.build as B
    assert B.COMPANIONS[0] == ("libsgp_exact_nuts_hip.so", ["sgp_exact_nuts.hip"], "sgp_exact_nuts.h")
    assert ("libsgp_exact_predict_hip.so", ["sgp_exact_predict.hip"], "sgp_exact_predict.h") in B.COMPANIONS
    assert [c[1] for c in B.COMPANIONS].count(["sgp_exact_predict.hip"]) == 1 and "sgp_exact_predict.hip" not in B.SOURCES


def test_the_digest_covers_the_new_library(lib, tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("_sgp_build_ep", os.path.join(ROOT, "generalised-gaussian-processes_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    (name, sources, header), = [c for c in b.COMPANIONS if c[0] == "libsgp_exact_predict_hip.so"]
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
    for edited in (work / "sgp_exact_predict.hip", work / "sgp_exact_predict.hpp", work / "sgp_exact_batch.hpp", work / "sgp_wg_dense.hpp",
                   work / "sgp_common.hpp", tmp_path / "include" / header):
        with open(edited, "a") as fh:
            fh.write("// a comment\n")
        after = b._companion_digest(b._digest(), sources, header)
        assert after != before, edited
        before = after


# ---------------------------------------------------------------------------------------------------------------- refusals, no device
def _predict_args(**bad):
    a = dict(ptr=8, T=5, P=2, N=10, d=2, kid=0, ws=8, nbytes=256, ldx=2)
    a.update(bad)
    p = C.c_void_p(a["ptr"])  # (the dummy 8 is never dereferenced: every call here fails validation first)
    return (p, 20, a["ldx"], p, 10, p, 10, a["ldx"], a["T"], None, None, None, p, a["P"], a["N"], a["d"], a["kid"], 1, p, p, p,
            C.c_void_p(a["ws"]), a["nbytes"], None)


def test_out_of_range_arguments_are_refused_on_the_host(lib):
    q = lib.sgp_exact_predict_batch_workspace_bytes
    assert q(2, 10, 2, 5) == 256 and q(2 ** 24 - 1, 128, 8, 32768) == 256
    assert q(2, 129, 2, 5) == 0 and q(2, 10, 9, 5) == 0 and q(2, 10, 2, 0) == 0 and q(2, 10, 2, 32769) == 0
    assert q(0, 10, 2, 5) == 0 and q(2 ** 24, 10, 2, 5) == 0 and q(2, 0, 2, 5) == 0
    for bad, status in ((dict(N=129), -2), (dict(d=9, ldx=9), -2), (dict(T=0), -1), (dict(T=32769), -2), (dict(P=2 ** 24), -2),
                        (dict(P=0), -1), (dict(kid=3), -1), (dict(kid=-1), -1), (dict(ptr=0), -1), (dict(ldx=1), -1),
                        (dict(nbytes=255), -3), (dict(ws=0), -3), (dict(N=129, ptr=0), -1)):
        assert lib.sgp_exact_predict_batch(*_predict_args(**bad)) == status, bad
        assert lib.sgp_ctx_exact_predict_batch(None, *_predict_args(**bad)) == status, bad
    assert lib.sgp_exact_predict_batch_occupancy(129, 0) == -2 and lib.sgp_exact_predict_batch_occupancy(0, 0) == -1
    assert lib.sgp_exact_predict_batch_occupancy(10, 3) == -1
    m = lib.sgp_exact_mixture_workspace_bytes
    assert m(1, 1) == 256 and m(0, 5) == 0 and m(3, 0) == 0 and m(3, 32769) == 0 and m(2 ** 24, 5) == 0
    p, z = C.c_void_p(8), None
    mix = lambda G=2, T=5, mean=p, y=p, lp=p, ws=p, nbytes=256: lib.sgp_exact_mixture_reduce(  # noqa: E731
        mean, p, p, p, G, T, y, p, p, lp, p, p, ws, nbytes, None)
    assert mix(G=0) == -1 and mix(T=0) == -1 and mix(T=32769) == -2 and mix(G=2 ** 24) == -2 and mix(mean=z) == -1
    assert mix(lp=z) == -1 and mix(nbytes=255) == -3 and mix(ws=z) == -3 and mix(G=2 ** 24, mean=z) == -1


# ---------------------------------------------------------------------------------------------------------------- the CPU double
@pytest.mark.parametrize("N,d,kernel", CELLS_A)
def test_the_double_meets_the_bound_at_the_edge_shapes(N, d, kernel):
    check_edge_cell(ExactPredictDouble(), _host, N, d, kernel)


@pytest.mark.parametrize("N,d", CELLS_B)
def test_the_double_meets_the_bound_at_the_t_edges(N, d):
    check_t_edges(ExactPredictDouble(), _host, N, d, same_bits=False)


def test_the_double_meets_the_derived_reduction_bounds():
    check_mixture(ExactPredictDouble(), _host)


def test_the_double_reports_failures_like_the_kernel():
    from test_exact_batch import bad_theta_rows
    rng = np.random.default_rng(4)
    X, y, Xs = rng.uniform(0, 10, (6, 2)), rng.standard_normal(6), rng.uniform(0, 10, (5, 2))
    e = ExactPredictDouble()
    mean, var, info = e.exact_predict_batch(X, y, bad_theta_rows(), Xs)
    assert info.tolist() == [0] + [1] * 7 and bool(mean[1:].isnan().all()) and bool(var[0].isfinite().all())
    with pytest.raises(ValueError):
        e.exact_predict_batch(X, y, bad_theta_rows(), Xs, ix=[1] * 8)
    for off in ([0, 3, 2, 8], [0, 4, 7], [1, 8]):
        with pytest.raises(ValueError):
            e.exact_mixture(mean, var, info, off)


# ---------------------------------------------------------------------------------------------------------------- the public layer
def _toy(B=3, N=12, d=2, S=5, T=7, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 10.0, (B, N, d))
    Y = rng.standard_normal((B, N))
    Xt = rng.uniform(0.0, 10.0, (B, T, d))
    Yt = rng.standard_normal((B, T))
    q = rng.uniform(-0.5, 0.8, (B, S, d + 2))
    return X, Y, Xt, Yt, q


def test_predict_exact_batch_shapes_and_the_numpy_formulas():
    X, Y, Xt, Yt, q = _toy()
    B, S, T = q.shape[0], q.shape[1], Xt.shape[1]
    eng = ExactPredictDouble()
    r = ggp_amd.predict_exact_batch(X, Y, q, Xt, Yt, kernel="matern32", engine=eng)
    assert isinstance(r, ggp_amd.ExactMixturePredictive)
    assert eng.calls["exact_predict_batch"] == 1 and eng.calls["exact_mixture"] == 1
    assert r.mean.shape == r.var.shape == r.logpdf.shape == r.mean_logpdf.shape == (B, T)
    assert r.draw_mean.shape == r.draw_var.shape == (B, S, T) and r.info.shape == (B, S) and r.kept.tolist() == [S] * B
    # every data set alone, with shared X / X_test given as 2-d arrays, is the same problem
    for b in range(B):
        rb = ggp_amd.predict_exact_batch(X[b], Y[b], q[b], Xt[b], Yt[b], kernel="matern32", engine=eng)
        assert np.allclose(rb.draw_mean[0], r.draw_mean[b], rtol=1e-12, atol=1e-13) and np.allclose(rb.logpdf[0], r.logpdf[b], rtol=1e-10)
    shared = ggp_amd.predict_exact_batch(X[0], Y, q, Xt[0], engine=eng)
    assert shared.mean.shape == (B, T) and shared.logpdf is None and shared.mean_logpdf is None
    with pytest.raises(ValueError):
        shared.nlpd()
    # theta = [exp, exp^2, exp^2 + jitter]; the moments and densities in numpy
    th = np.concatenate([np.exp(q[..., :-2]), np.exp(q[..., -2:]) ** 2], -1)
    m, v, _ = eng.exact_predict_batch(X, Y, th.reshape(B * S, -1), Xt, ix=np.repeat(np.arange(B), S), iy=np.repeat(np.arange(B), S),
                                      ixs=np.repeat(np.arange(B), S), kernel="matern32")
    assert np.array_equal(m.numpy().reshape(B, S, T), r.draw_mean) and np.array_equal(v.numpy().reshape(B, S, T), r.draw_var)
    assert np.allclose(r.mean, r.draw_mean.mean(1), rtol=1e-13) and np.allclose(r.var, (r.draw_var + (r.draw_mean - r.mean[:, None]) ** 2).mean(1))
    l = -0.5 * np.log(2 * np.pi * r.draw_var) - 0.5 * (Yt[:, None] - r.draw_mean) ** 2 / r.draw_var
    assert np.allclose(r.mean_logpdf, l.mean(1), rtol=1e-12) and np.allclose(r.logpdf, np.log(np.exp(l).mean(1)), rtol=1e-10)
    for Y_std in (1.0, 2.5):
        assert np.allclose(r.nlpd(Y_std), -np.log(np.exp(l).mean(1)).mean(1) + np.log(Y_std), rtol=1e-10)
        assert np.allclose(r.rmse(Yt, Y_std), Y_std * np.sqrt(((r.draw_mean.mean(1) - Yt) ** 2).mean(1)), rtol=1e-12)
        # the reference's metric averages log densities over draws and test points (and rounds to three decimals)
        for b in range(B):
            want = metrics.negative_log_predictive_mixture_density(torch.as_tensor(Yt[b]), r.draw_mean[b], np.sqrt(r.draw_var[b]), Y_std)
            assert abs(float(want) - (-r.mean_logpdf[b].mean() + np.log(Y_std))) <= 5.01e-4
    jit = ggp_amd.predict_exact_batch(X, Y, q, Xt, kernel="matern32", jitter=0.25, engine=eng)
    th[..., -1] += 0.25
    m2, v2, _ = eng.exact_predict_batch(X[0], Y[0], th[0], Xt[0], kernel="matern32")
    assert np.array_equal(v2.numpy(), jit.draw_var[0]) and not np.array_equal(jit.draw_var, r.draw_var)


def test_noise_floor_nan_rows_and_the_callers_array():
    X, Y, Xt, Yt, q = _toy(B=2, S=4)
    q[0, 1, -1] = np.log(1e-3)    # sig_n^2 = 1e-6 < 1e-4: predicted at sig_n = 0.01
    q[1, 2] = np.nan              # a chain that had no start
    before = q.copy()
    eng = ExactPredictDouble()
    r = ggp_amd.predict_exact_batch(X, Y, q, Xt, Yt, engine=eng)
    assert np.array_equal(q, before, equal_nan=True)
    assert r.kept.tolist() == [4, 3] and r.info[1, 2] == 1 and r.info.sum() == 1 and np.isnan(r.draw_mean[1, 2]).all()
    assert np.isfinite(r.mean).all() and np.isfinite(r.logpdf).all()
    assert np.allclose(r.mean[1], r.draw_mean[1, [0, 1, 3]].mean(0), rtol=1e-13)
    th = np.concatenate([np.exp(q[0, 1, :2]), [np.exp(q[0, 1, 2]) ** 2, 0.01 ** 2]])
    _, v, _ = eng.exact_predict_batch(X[0], Y[0], th[None], Xt[0])
    assert np.array_equal(v.numpy()[0], r.draw_var[0, 1])
    q[0, 1, -1] = np.log(0.011)   # just above the floor: taken as it is
    r2 = ggp_amd.predict_exact_batch(X, Y, q, Xt, Yt, engine=eng)
    th[-1] = np.exp(q[0, 1, -1]) ** 2
    assert np.array_equal(eng.exact_predict_batch(X[0], Y[0], th[None], Xt[0])[1].numpy()[0], r2.draw_var[0, 1])


def test_results_carry_what_predict_needs():
    rng = np.random.default_rng(5)
    B, N = 2, 10
    X = np.sort(rng.uniform(0.0, 10.0, (N, 1)), 0)
    Y = np.sin(X[:, 0])[None] + 0.1 * rng.standard_normal((B, N))
    Xt, Yt = rng.uniform(0.0, 10.0, (6, 1)), rng.standard_normal((B, 6))
    eng = ExactPredictDouble()
    post = ggp_amd.sample_exact_nuts_batch(X, Y, 6, 8, chains=2, seed=1, jitter=1e-3, engine=eng)
    assert post.kernel == "rbf" and post.jitter == 1e-3 and post.engine is eng and post.X.shape == (N, 1) and post.Y.shape == (B, N)
    r = post.predict(Xt, Yt, thin=2)
    assert r.draw_mean.shape == (B, 2 * 3, 6) and r.kept.tolist() == [6, 6] and np.isfinite(r.nlpd()).all()
    want = ggp_amd.predict_exact_batch(X, Y, post.samples[:, :, ::2].reshape(B, 6, 3), Xt, Yt, jitter=1e-3, engine=eng)
    assert np.array_equal(want.draw_mean, r.draw_mean) and np.array_equal(want.logpdf, r.logpdf)
    assert post.predict(Xt).draw_mean.shape == (B, 12, 6)
    with pytest.raises(ValueError):
        post.predict(Xt, thin=0)
    # a result constructed without the new fields (as before they existed) still works; predict says what is missing
    old = ggp_amd.ExactNutsResult(traces=[], samples=post.samples, stats=post.stats, seconds=post.seconds, evaluations=post.evaluations,
                                  draws=post.draws, info=post.info, seeds=post.seeds, starts=post.starts, launches=1, wall_clock_secs=0.0)
    assert old.posterior_mean().shape == (B, 3) and old.X is None
    with pytest.raises(ValueError, match="does not carry the data"):
        old.predict(Xt)
    fit = ggp_amd.fit_ml2(X, Y, theta0=[1.0, 1.0, 0.1], bounds=np.array([(1e-2, 1e3), (1e-5, 1e5), (1e-5, 1e5)]), n_restarts=1, seed=0,
                          engine=eng)
    p = fit.predict(Xt, Yt)
    assert p.draw_mean.shape == (B, 1, 6) and p.kept.tolist() == [1, 1] and np.isfinite(p.nlpd()).all() and np.isfinite(p.rmse(Yt)).all()
    assert np.array_equal(p.mean, p.draw_mean[:, 0])   # S = 1: the plug-in predictive at theta, no exp and no floor
    m, _, _ = eng.exact_predict_batch(X, Y, fit.theta, Xt, iy=[0, 1])
    assert np.array_equal(m.numpy(), p.mean)
    bare = ggp_amd.Ml2Result(theta=fit.theta, lml=fit.lml, n_evals=fit.n_evals, theta_all=fit.theta_all, lml_all=fit.lml_all,
                             converged=fit.converged, n_iter=fit.n_iter, n_batches=1)
    with pytest.raises(ValueError, match="does not carry the data"):
        bare.predict(Xt)


def test_experiment_holdout_flag_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4", "--hmc", "--hmc_chains", "2", "--hmc_tune", "8",
            "--hmc_draws", "6"]
    eng = ExactPredictDouble()
    s = mod.main(base + ["--holdout", "5", "--out", str(tmp_path / "held")], engine=eng)
    new = ["%s_%s_%s" % (c, m, k) for c in ("size", "noise") for m in ("ml2", "hmc") for k in ("nlpd", "rmse")]
    for k in new:
        assert len(s[k]) == 1 and np.isfinite(s[k]).all(), k
    z = np.load(tmp_path / "held" / "hyperparameter_identification.npz")
    assert z["size_learn_nlpd"].shape == z["size_hmc_rmse"].shape == (1, 2) and z["size_learn_ls"].shape == (1, 2)
    assert eng.calls["exact_predict_batch"] == 4  # per cell: the plug-in and the mixture
    assert set(new) <= set(json.load(open(tmp_path / "held" / "hyperparameter_identification.json")))
    # --holdout 0 (the default): exactly today's keys, and the engine's predictive is never called
    eng0 = ExactPredictDouble()
    s0 = mod.main(base + ["--out", str(tmp_path / "plain")], engine=eng0)
    s00 = mod.main(base + ["--holdout", "0", "--out", str(tmp_path / "zero")], engine=ExactPredictDouble())
    assert set(s0) == set(s00) == set(s) - set(new) and eng0.calls["exact_predict_batch"] == 0
    z0 = np.load(tmp_path / "plain" / "hyperparameter_identification.npz")
    assert set(z0.files) == set(z.files) - {"%s_%s_%s" % (c, m, k) for c in ("size", "noise") for m in ("learn", "hmc") for k in ("nlpd", "rmse")}
    assert np.array_equal(z0["size_learn_ls"], np.load(tmp_path / "zero" / "hyperparameter_identification.npz")["size_learn_ls"])


# ---------------------------------------------------------------------------------------------------------------- the host program
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_mixture_arithmetic_on_the_host_under_asan_ubsan(tmp_path):
    """tests/native/exact_mixture_host.cpp (its own main, csrc/sgp_exact_predict.hpp) on the cells of family (g) -- a group of one draw
    (n = 1) and a group whose draws have all failed (n = 0) among them -- against long double under the derived bounds."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on CPU-only hosts, never on a GPU box")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "exact_mixture_host_asan")
    subprocess.run([gxx, "-O1", "-std=c++17"] + SAN + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "exact_mixture_host.cpp")],
                   check=True, timeout=300)
    mean, var, info, off, Y = mixture_case(ExactPredictDouble(), _host)
    m, v, i = mean.numpy(), var.numpy(), info.numpy()
    m, v = np.nan_to_num(m, nan=0.0), np.nan_to_num(v, nan=1.0)  # (the failed draws' rows: never read; the text format has no NaN)
    G, T, P = 4, m.shape[1], m.shape[0]
    for has_y in (1, 0):
        case = tmp_path / ("case%d.txt" % has_y)
        rows = ["%d %d %d %d" % (G, T, P, has_y), " ".join(map(str, off)), " ".join(str(int(k)) for k in i)]
        rows += [" ".join(float(x).hex() for x in a.reshape(-1)) for a in ((m, v, Y) if has_y else (m, v))]
        case.write_text("\n".join(rows) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "exact mixture ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
        got = np.array([[float(w[2])] + [float.fromhex(x) for x in w[3:]] for w in map(str.split, r.stdout.splitlines()[:-1])]).reshape(G, T, 5)
        assert got[:, 0, 0].tolist() == [1, 2, 64, 0] and np.isnan(got[3, :, 1:]).all()
        keys = ("mean", "var", "logpdf", "mean_logpdf")[:4 if has_y else 2]
        if not has_y:
            assert np.isnan(got[:, :, 3:]).all()
        for g in range(3):
            ref = mixture_reference(m[off[g]:off[g + 1]], v[off[g]:off[g + 1]], i[off[g]:off[g + 1]], Y[g] if has_y else None)
            assert_mixture_close({k: got[g, :, 1 + j] for j, k in enumerate(keys)}, ref, "group %d" % g)
