"""CPU: GPR_HMC (reference models/gpr_hmc.py) over the exact-GP test double -- the double against scikit-learn, ExactHmcTarget
against central differences and a hand-written density, a quadrature posterior pin, the model surface and the GPR branch of
full_mixture_posterior_predictive."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from exact_double import ExactDouble, exact_reference, hand_logp

import ggp_amd

T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731


def sklearn_cells():
    z = np.load(os.path.join(GOLDEN_DIR, "sklearn", "exact_lml.npz"))
    cells = []
    for c in range(int(z["n_cells"])):
        p = "c%d_" % c
        ls, sf2, s2 = z[p + "ls"], float(z[p + "sf2"]), float(z[p + "s2"])
        g = z[p + "grad_log"]  # d/dlog sf2, d/dlog ls_1..d, d/dlog s2
        cells.append({"X": z[p + "X"], "y": z[p + "y"], "ls": ls, "sf2": sf2, "s2": s2, "kernel": str(z[p + "kernel"]),
                      "F": float(z[p + "F"]), "g_sf2": g[0] / sf2, "g_ls": g[1:-1] / ls, "g_s2": g[-1] / s2})
    return cells


def quadrature_posterior(X, y, n=56, lo=(-3.0, -5.0, -5.0), hi=(4.0, 5.0, 1.0)):
    """Mean, covariance and fourth central moments of (log ls, log sig_f, log sig_n) under ExactHmcTarget's density (d = 1),
    by the midpoint rule on an n^3 grid, batched Cholesky in float64."""
    X = T(X).reshape(-1, 1)
    y = T(y).reshape(-1)
    N = X.shape[0]
    axes = [torch.linspace(a, b, n, dtype=torch.float64) for a, b in zip(lo, hi)]
    G = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    r2u = (X - X.T) ** 2
    lps = []
    for ch in torch.split(G, 16384):
        ls, sf, sn = torch.exp(ch[:, 0]), torch.exp(ch[:, 1]), torch.exp(ch[:, 2])
        A = sf[:, None, None] ** 2 * torch.exp(-0.5 * r2u[None] / ls[:, None, None] ** 2) + (sn ** 2)[:, None, None] * torch.eye(N, dtype=torch.float64)
        L, info = torch.linalg.cholesky_ex(A)
        a = torch.linalg.solve_triangular(L, y[None, :, None].expand(len(ch), N, 1), upper=False)[..., 0]
        F = -0.5 * (a * a).sum(1) - torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1) - 0.5 * N * math.log(2 * math.pi)
        F = torch.where(info == 0, F, torch.full_like(F, -math.inf))
        lp = (torch.log(ls) - ls) + 2 * math.log(2 / math.pi) - torch.log1p(sf ** 2) - torch.log1p(sn ** 2) + ch.sum(1)
        lps.append(F + lp)
    lp = torch.cat(lps)
    w = torch.exp(lp - lp.max())
    w = w / w.sum()
    mean = (w[:, None] * G).sum(0)
    C = G - mean
    cov = (w[:, None, None] * C[:, :, None] * C[:, None, :]).sum(0)
    m4 = (w[:, None] * C ** 4).sum(0)
    # the grid must hold the mass: the boundary faces carry a negligible share
    edge = ((G == G.min(0).values) | (G == G.max(0).values)).any(1)
    assert float(w[edge].sum()) < 1e-4, float(w[edge].sum())
    return {"mean": mean.numpy(), "cov": cov.numpy(), "m4": m4.numpy()}


def pin_data():
    rng = np.random.default_rng(7)
    X = np.sort(rng.uniform(-3.0, 3.0, 20))
    y = np.sin(X) + 0.2 * rng.standard_normal(20)
    return X[:, None], y


def test_double_matches_sklearn():
    for c in sklearn_cells():
        r = exact_reference(c["X"], c["y"], c["ls"], c["sf2"], c["s2"], c["kernel"])
        assert r["info"] == 0
        assert abs(r["F"] - c["F"]) <= 1e-12 * abs(c["F"]), (c["kernel"], r["F"], c["F"])
        gmax = max(1.0, float(np.abs(c["g_ls"]).max()), abs(c["g_sf2"]), abs(c["g_s2"]))
        assert np.abs(r["g_ls"].numpy() - c["g_ls"]).max() <= 1e-10 * gmax, (c["kernel"], r["g_ls"], c["g_ls"])
        assert abs(r["g_sf2"] - c["g_sf2"]) <= 1e-10 * gmax
        assert abs(r["g_s2"] - c["g_s2"]) <= 1e-10 * gmax


@pytest.mark.parametrize("kernel", ["rbf", "matern32", "matern52"])
def test_target_gradient_against_central_differences_and_hand_density(kernel):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 3))
    y = np.cos(X @ np.array([1.0, -0.5, 0.3])) + 0.1 * rng.standard_normal(40)
    tgt = ggp_amd.ExactHmcTarget(T(X), T(y), kernel=kernel, engine=ExactDouble())
    assert tgt.ndim == 5 and tgt.start() == [math.log(2.0)] * 3 + [0.0, 0.0]
    th = np.array([0.3, 0.9, -0.2, 0.1, -1.2])
    lp, g = tgt.logp_and_grad(th)
    assert abs(lp - hand_logp(X, y, th, kernel)) < 1e-10 * abs(lp)
    assert abs(tgt.logp(th) - lp) < 1e-12 * abs(lp)
    h = 1e-5
    for k in range(5):
        e = np.zeros(5)
        e[k] = h
        fd = (tgt.logp(th + e) - tgt.logp(th - e)) / (2 * h)
        assert abs(fd - g[k]) < 1e-6 * max(1.0, abs(g[k])), (kernel, k, fd, g[k])
    c = tgt.constrain(th)
    assert set(c) == {"ls", "sig_f", "sig_n"} and abs(c["sig_n"] - math.exp(-1.2)) < 1e-15


def test_target_failure_is_minus_inf_not_an_exception():
    X = np.zeros((6, 2))  # identical rows: A = sf2 11^T + s2 I is singular at s2 = 0 (exp(-inf) noise below)
    tgt = ggp_amd.ExactHmcTarget(T(X), T(np.ones(6)), engine=ExactDouble())
    lp, g = tgt.logp_and_grad([0.0, 0.0, 0.0, -300.0 + 1e-9])
    assert lp == -math.inf and g == [0.0] * 4
    lp, g = tgt.logp_and_grad([0.0, 0.0, 0.0, -200.0])
    assert lp == -math.inf and g == [0.0] * 4
    assert tgt.logp([float("nan"), 0.0, 0.0, 0.0]) == -math.inf


def test_quadrature_posterior_pin_on_the_double():
    from test_posterior_pin import check_moments
    X, y = pin_data()
    P = quadrature_posterior(X, y)
    tgt = ggp_amd.ExactHmcTarget(T(X), T(y), engine=ExactDouble())
    tr = ggp_amd.sample_nuts(tgt, 1200, 400, seed=5)
    assert np.asarray(tr.get_sampler_stats("diverging")).mean() <= 0.01
    th = np.log(np.stack([np.asarray(tr["ls"]).reshape(-1), tr["sig_f"], tr["sig_n"]], 1))
    check_moments(th, P, "sample_nuts / exact double")


def _model(N=60, d=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    return ggp_amd.GPR_HMC(T(X), T(y), ggp_amd.GaussianLikelihood(), engine=ExactDouble(), seed=1), X, y


def test_gpr_hmc_surface():
    m, X, y = _model()
    trace, step, perf = m.train_model()
    assert len(trace) == 10 and set(trace.varnames) == {"ls", "sig_f", "sig_n"}
    assert np.asarray(trace["ls"]).shape == (10, 2) and np.asarray(trace["sig_f"]).shape == (10,)
    assert len(step) == 1 and step[0] > 0 and len(perf) == 1 and perf[0] > 0
    with pytest.raises(ValueError, match="input_dim"):
        m.sample_optimal_variational_hyper_dist(2, 3, 2)
    with pytest.raises(ValueError, match="4096"):
        ggp_amd.GPR_HMC(torch.zeros(4097, 1, dtype=torch.float64), torch.zeros(4097, dtype=torch.float64), ggp_amd.GaussianLikelihood(),
                        engine=ExactDouble())
    # ExactGP semantics: prior in training mode, exact posterior in eval mode, likelihood adds the noise
    m.train()
    prior = m(T(X[:5]))
    assert torch.allclose(prior.covariance_matrix.diagonal(), torch.full((5,), float(m.covar_module.outputscale.detach()), dtype=torch.float64))
    m.eval()
    m.likelihood.eval()
    f = m(T(X[:5]))
    yv = m.likelihood(f)
    s2 = float(m.likelihood.noise.detach())
    assert torch.allclose(yv.covariance_matrix - f.covariance_matrix, s2 * torch.eye(5, dtype=torch.float64), atol=1e-12)


class _IndefiniteAt(ExactDouble):
    """The double, except that the predictive at sf2 == 49 comes back indefinite beyond the 1e-2 gate."""

    def exact_predict(self, Xs, X, ls, sf2, s2, factors, kernel="rbf", pred_noise=True, full_cov=False):
        mean, var, cov = super().exact_predict(Xs, X, ls, sf2, s2, factors, kernel, pred_noise, full_cov)
        if abs(sf2 - 49.0) < 1e-9 and cov is not None:
            cov = cov - 1e3 * torch.eye(cov.shape[0], dtype=torch.float64)
        return mean, var, cov


def test_full_mixture_gpr_branch(capsys):
    m, X, y = _model(seed=2)
    trace, _, _ = m.train_model()
    trace[0]["sig_n"] = 0.005        # sig_n^2 < 1e-4: floored to 0.01 in the trace row itself
    trace[1]["sig_f"] = 7.0          # a predictive whose covariance fails cholesky(cov + 1e-2 I) is skipped
    m._exact_target().engine = eng = _IndefiniteAt()
    n0 = eng.calls["exact_predict"]
    preds = ggp_amd.full_mixture_posterior_predictive(m, T(X[:7]), trace)
    assert trace[0]["sig_n"] == 0.01
    out = capsys.readouterr().out
    assert "Not psd for sample 1" in out
    assert len(preds) == 9 and eng.calls["exact_predict"] - n0 == 10
    for p in preds:
        assert p.loc.shape == (7,) and p.covariance_matrix.shape == (7, 7)
    # draw 0's predictive is the double's at the floored noise
    th = trace[0]
    r = eng.exact_eval(m._exact_target().X, m._exact_target().y, list(th["ls"]), th["sig_f"] ** 2, 0.01 ** 2, want_grad=False,
                       want_factors=True)
    mu, _, cov = eng.exact_predict(T(X[:7]), m._exact_target().X, list(th["ls"]), th["sig_f"] ** 2, 1e-4, r["factors"], full_cov=True)
    assert torch.allclose(preds[0].loc, mu, atol=1e-12) and torch.allclose(preds[0].covariance_matrix, cov, atol=1e-12)
    rm = ggp_amd.rmse(torch.stack([p.loc for p in preds]).mean(0), T(y[:7]), torch.tensor(1.0))
    assert math.isfinite(float(rm))
