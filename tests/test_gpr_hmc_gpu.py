"""GPU: sgp_exact_eval / sgp_exact_predict (csrc/sgp_exact.hip) against the float64 CPU yardstick of tests/exact_double.py and the
scikit-learn fixture, bit reproducibility, the failure paths, the posterior pin on the device target and GPR_HMC end to end."""
import math

import numpy as np
import pytest
import torch

from conftest import dev
from exact_double import ExactDouble, exact_reference
from test_gpr_hmc import T, pin_data, quadrature_posterior, sklearn_cells

import ggp_amd

pytestmark = pytest.mark.gpu

# (N, d, kernel): every N and d of the issue's grid appears, every kernel at small, middle and large N
CELLS = [(1, 1, "rbf"), (2, 6, "matern32"), (63, 8, "matern52"), (64, 13, "rbf"), (65, 32, "matern32"), (277, 6, "matern52"),
         (455, 13, "rbf"), (927, 8, "matern32"), (1439, 11, "rbf"), (2048, 8, "matern52"), (4096, 8, "rbf"), (4096, 6, "matern32")]


def problem(N, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X[:, 0] + 0.5 * X.sum(1) / math.sqrt(d)) + 0.3 * rng.standard_normal(N)
    ls = list(rng.gamma(2.0, 1.0, d) + 0.5 * math.sqrt(d))  # around the Gamma(2, 1) prior, scaled with the input norm
    sf2 = float(rng.uniform(0.5, 2.0))
    s2 = float(rng.uniform(0.05, 0.5))
    return X, y, ls, sf2, s2


def cond_of(X, ls, sf2, s2, kernel):
    from exact_double import kernel_parts
    K = kernel_parts(X, X, ls, sf2, kernel)[0] + s2 * torch.eye(X.shape[0], dtype=torch.float64)
    ev = torch.linalg.eigvalsh(K)
    return float(ev[-1] / ev[0])


def check_against(r, ref, N, cond, what):
    F, Fr = r["F"], ref["F"]
    assert abs(F - Fr) <= 1e-10 * (abs(Fr) + N), "%s: F %.17g vs %.17g (cond %.3g)" % (what, F, Fr, cond)
    g = np.array(r["ls"] + [r["sf2"], r["s2"]])
    gr = np.concatenate([ref["g_ls"].numpy(), [ref["g_sf2"], ref["g_s2"]]])
    if cond <= 1e8:
        tol = 1e-8 * max(1.0, float(np.abs(gr).max()))
        assert np.abs(g - gr).max() <= tol, "%s: gradient off by %.3g > %.3g (cond %.3g)\n%s\n%s" % (
            what, np.abs(g - gr).max(), tol, cond, g, gr)


@pytest.mark.parametrize("N,d,kernel", CELLS)
def test_exact_eval_matches_the_float64_yardstick(engine, N, d, kernel):
    X, y, ls, sf2, s2 = problem(N, d, N + 7 * d)
    r = engine.exact_eval(dev(X, engine), dev(y, engine), ls, sf2, s2, kernel=kernel)
    assert r["info"] == 0, r["info"]
    ref = exact_reference(X, y, ls, sf2, s2, kernel)
    cond = cond_of(X, ls, sf2, s2, kernel) if N <= 1500 else 0.0  # (the larger cells: N sf2 / s2 < 1e6 bounds it)
    check_against(r, ref, N, cond, "N=%d d=%d %s" % (N, d, kernel))
    out = r["out"]
    assert abs(out[1] - ref["quad"]) <= 1e-10 * (abs(ref["quad"]) + N)
    assert abs(out[2] - ref["logdet"]) <= 1e-10 * (abs(ref["logdet"]) + N)
    assert abs(out[3] - ref["trinv"]) <= 1e-10 * abs(ref["trinv"])


def test_exact_eval_matches_sklearn(engine):
    for c in sklearn_cells():
        r = engine.exact_eval(dev(c["X"], engine), dev(c["y"], engine), list(c["ls"]), c["sf2"], c["s2"], kernel=c["kernel"])
        assert r["info"] == 0
        N = c["X"].shape[0]
        assert abs(r["F"] - c["F"]) <= 1e-10 * (abs(c["F"]) + N), (c["kernel"], r["F"], c["F"])
        g = np.array(r["ls"] + [r["sf2"], r["s2"]])
        gr = np.concatenate([c["g_ls"], [c["g_sf2"], c["g_s2"]]])
        assert np.abs(g - gr).max() <= 1e-8 * max(1.0, float(np.abs(gr).max())), (c["kernel"], g, gr)


def test_same_bits_on_every_call_and_every_stream():
    X, y, ls, sf2, s2 = problem(927, 8, 1)
    e0 = ggp_amd.HipEngine()
    Xd, yd = dev(X, e0), dev(y, e0)

    def bits(eng, stream=None):
        if stream is None:
            r = eng.exact_eval(Xd, yd, ls, sf2, s2)
        else:
            with torch.cuda.stream(stream):
                r = eng.exact_eval(Xd, yd, ls, sf2, s2)
        return np.array(r["out"] + r["ls"] + [r["sf2"], r["s2"]]).view(np.uint64)

    first = bits(e0)
    for _ in range(19):
        assert np.array_equal(bits(e0), first)
    a, b = ggp_amd.HipEngine(own_context=True), ggp_amd.HipEngine(own_context=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    assert np.array_equal(bits(a, sa), first) and np.array_equal(bits(b, sb), first)


def test_singular_matrix_is_reported_not_raised(engine):
    rng = np.random.default_rng(2)
    X = rng.standard_normal((40, 3))
    X[20:] = X[:20]  # duplicated rows
    y = rng.standard_normal(40)
    r = engine.exact_eval(dev(X, engine), dev(y, engine), [1.0, 1.0, 1.0], 1.0, 1e-300)
    assert r["info"] != 0
    tgt = ggp_amd.ExactHmcTarget(T(X).to(engine.device), T(y).to(engine.device), engine=engine)
    lp, g = tgt.logp_and_grad([0.0, 0.0, 0.0, 0.0, -200.0])
    assert lp == -math.inf and g == [0.0] * 5
    assert tgt.logp([0.0, 0.0, 0.0, 0.0, -200.0]) == -math.inf


def test_out_of_range_arguments_raise_a_status_error(engine):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=engine.device)  # noqa: E731
    with pytest.raises(ggp_amd.SgpStatusError) as ei:
        engine.exact_eval(z(4097, 2), z(4097), [1.0, 1.0], 1.0, 0.1)
    assert ei.value.status == -2
    with pytest.raises(ggp_amd.SgpStatusError) as ei:
        engine.exact_eval(z(10, 33), z(10), [1.0] * 33, 1.0, 0.1)
    assert ei.value.status == -2
    block = [1.0, 1.0, 1.0, 0.0, 1.0, 0.0] + [0.0] * 27  # a valid one-term composite block: still refused (out of scope)
    with pytest.raises(ggp_amd.SgpStatusError) as ei:
        engine.exact_eval(z(10, 2), z(10), block, 1.0, 0.1, kernel="composite")
    assert ei.value.status == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("Tn", [1, 100, 1000])
def test_exact_predict_matches_the_yardstick(engine, Tn):
    X, y, ls, sf2, s2 = problem(455, 6, 11)
    rng = np.random.default_rng(Tn)
    Xs = rng.standard_normal((Tn, 6))
    kernel = {1: "rbf", 100: "matern32", 1000: "matern52"}[Tn]
    r = engine.exact_eval(dev(X, engine), dev(y, engine), ls, sf2, s2, kernel=kernel, want_grad=False, want_factors=True)
    assert r["info"] == 0
    for noise in (True, False):
        mu, var, cov = engine.exact_predict(dev(Xs, engine), dev(X, engine), ls, sf2, s2, r["factors"], kernel=kernel, pred_noise=noise,
                                            full_cov=True)
        dbl = ExactDouble()
        rr = dbl.exact_eval(T(X), T(y), ls, sf2, s2, kernel=kernel, want_grad=False, want_factors=True)
        mr, vr, cr = dbl.exact_predict(T(Xs), T(X), ls, sf2, s2, rr["factors"], kernel=kernel, pred_noise=noise, full_cov=True)
        assert float((mu.cpu() - mr).abs().max()) <= 1e-9 * max(1.0, float(mr.abs().max()))
        assert float((var.cpu() - vr).abs().max()) <= 1e-9 * sf2
        assert float((cov.cpu() - cr).abs().max()) <= 1e-9 * sf2
        assert torch.allclose(torch.diagonal(cov).cpu(), var.cpu(), rtol=0, atol=1e-12 * sf2)


def test_quadrature_posterior_pin_on_the_device_target(engine):
    from test_posterior_pin import check_moments
    X, y = pin_data()
    P = quadrature_posterior(X, y)
    tgt = ggp_amd.ExactHmcTarget(T(X).to(engine.device), T(y).to(engine.device), engine=engine)
    tr = ggp_amd.sample_nuts(tgt, 1200, 400, seed=5)
    assert np.asarray(tr.get_sampler_stats("diverging")).mean() <= 0.01
    th = np.log(np.stack([np.asarray(tr["ls"]).reshape(-1), tr["sig_f"], tr["sig_n"]], 1))
    check_moments(th, P, "sample_nuts / device exact target")


def test_gpr_hmc_end_to_end_concrete_shape(engine, capsys):
    rng = np.random.default_rng(927)
    X = rng.standard_normal((1030, 8))
    f = np.sin(X[:, 0]) + 0.5 * X[:, 1] * X[:, 2] + 0.3 * X[:, 3:].sum(1)
    y = f + 0.2 * rng.standard_normal(1030)
    y = (y - y.mean()) / y.std()
    Xtr, ytr, Xte, yte = X[:927], y[:927], X[927:], y[927:]
    m = ggp_amd.GPR_HMC(dev(Xtr, engine), dev(ytr, engine), ggp_amd.GaussianLikelihood(), engine=engine, seed=3)
    trace, step, perf = m.train_model()
    assert len(trace) == 10 and step[0] > 0 and perf[0] > 0
    preds = ggp_amd.full_mixture_posterior_predictive(m, dev(Xte, engine), trace)
    assert len(preds) == 10, capsys.readouterr().out  # a well-posed problem: no draw is skipped
    mu = torch.stack([p.loc.cpu() for p in preds]).mean(0)
    rm = float(ggp_amd.rmse(mu, T(yte), torch.tensor(1.0)))
    nl = float(ggp_amd.nlpd_mixture(preds, dev(yte, engine), torch.tensor(1.0)))
    assert math.isfinite(rm) and rm < 1.0 and math.isfinite(nl)
    dbl = ExactDouble()
    for i, p in enumerate(preds):
        th = trace[i]
        ls, sf2, s2 = list(np.asarray(th["ls"]).reshape(-1)), float(th["sig_f"]) ** 2, float(th["sig_n"]) ** 2
        rr = dbl.exact_eval(T(Xtr), T(ytr), ls, sf2, s2, want_grad=False, want_factors=True)
        mr, _, cr = dbl.exact_predict(T(Xte), T(Xtr), ls, sf2, s2, rr["factors"], full_cov=True)
        assert float((p.loc.cpu() - mr).abs().max()) <= 1e-9 * max(1.0, float(mr.abs().max())), i
        assert float((p.covariance_matrix.cpu() - cr).abs().max()) <= 1e-9 * max(1.0, float(cr.abs().max())), i
