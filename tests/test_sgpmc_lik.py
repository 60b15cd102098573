"""CPU: ``SgpmcTarget(likelihood=...)`` over the CPU double against torch autograd of a dense statement of the density, the
label / count checks, the predictive moments against direct sampling, and the argument checks of the two new entry points (which
need no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ggp_amd
from ggp_amd.sgp_hmc import likelihood_moments
from sgpmc_lik_double import SgpmcLikOracleEngine

NEW = ("bernoulli", "bernoulli_logit", "poisson")
JITTER = 1e-5


def problem(lik, N=40, M=6, d=2, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, d))
    Z = rng.uniform(-2.0, 2.0, (M, d))
    X[:2] = Z[:2]                                  # data on inducing inputs
    f = np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, 1])
    if lik == "poisson":
        y = rng.poisson(np.exp(f)).astype(np.float64)
    elif lik == "gaussian":
        y = f + 0.2 * rng.standard_normal(N)
    else:
        y = (f + 0.3 * rng.standard_normal(N) > 0).astype(np.float64)      # {0, 1}: the target maps them
    return torch.as_tensor(X), torch.as_tensor(y), torch.as_tensor(Z)


def logp_dense(q, X, y, Z, lik):
    """The density of ``SgpmcTarget(likelihood=lik)`` stated densely: GPflow's conditional with q_sqrt = None, white = True, the
    likelihood's variational expectation on the 20-point rule, v ~ N(0, I), softplus transforms, Gamma(2, 1) priors at the
    constrained values and log sigmoid(x) for each transform.  y in {-1, +1} for the Bernoulli links."""
    M, d = Z.shape
    sp = torch.nn.functional.softplus
    sf2, ls, v = sp(q[0]), sp(q[1:1 + d]), q[1 + d:]
    r2 = lambda a, b: (((a / ls)[:, None, :] - (b / ls)[None, :, :]) ** 2).sum(-1)
    K = sf2 * torch.exp(-0.5 * r2(Z, Z)) + JITTER * torch.eye(M, dtype=torch.float64)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(K), sf2 * torch.exp(-0.5 * r2(Z, X)), upper=False)
    mu, var = A.T @ v, sf2 - (A * A).sum(0)
    if lik == "poisson":
        ell = y * mu - torch.exp(mu + 0.5 * var) - torch.lgamma(y + 1.0)
    else:
        gx, gw = np.polynomial.hermite.hermgauss(20)
        gx, gw = torch.as_tensor(gx * math.sqrt(2.0)), torch.as_tensor(gw / math.sqrt(math.pi))
        z = y[:, None] * (mu[:, None] + torch.sqrt(var)[:, None] * gx[None, :])
        ell = ((torch.special.log_ndtr(z) if lik == "bernoulli" else torch.nn.functional.logsigmoid(z)) * gw).sum(1)
    F = ell.sum() - 0.5 * (v @ v) - 0.5 * M * math.log(2.0 * math.pi)
    cons = torch.cat([sf2.reshape(1), ls])
    return F + (torch.log(cons) - cons).sum() + torch.nn.functional.logsigmoid(q[:1 + d]).sum()


@pytest.mark.parametrize("want_gz", [False, True])
@pytest.mark.parametrize("lik", NEW)
def test_target_matches_autograd_of_the_dense_statement(lik, want_gz):
    X, y, Z = problem(lik)
    t = ggp_amd.SgpmcTarget(X, y, Z, jitter=JITTER, engine=SgpmcLikOracleEngine(), likelihood=lik)
    d, M = 2, 6
    assert t.ndim == d + 1 + M and len(t.start()) == t.ndim and "noise_variance" not in t.constrain(t.start())
    y_pm = torch.where(y > 0, 1.0, -1.0).to(torch.float64) if lik != "poisson" else y
    rng = np.random.default_rng(5)
    for k in range(3):
        q = np.concatenate([np.asarray(t.start()[:1 + d]) + 0.3 * rng.standard_normal(1 + d), (0.0, 1.0, 3.0)[k] * rng.standard_normal(M)])
        qt = torch.tensor(q, requires_grad=True)
        Zt = Z.clone().requires_grad_(True)
        lp = logp_dense(qt, X, y_pm, Zt, lik)
        gq, gz = torch.autograd.grad(lp, (qt, Zt))
        r = t.logp_and_grad(q, want_gz=want_gz)
        lp = float(lp.detach())
        assert abs(r[0] - lp) <= 1e-10 * (1.0 + abs(lp))
        assert np.allclose(np.asarray(r[1]), gq.numpy(), rtol=1e-8, atol=1e-8 * (1.0 + float(gq.abs().max())))
        assert abs(t.logp(q) - r[0]) <= 1e-12 * (1.0 + abs(r[0]))
        if want_gz:
            assert np.allclose(r[2].numpy(), gz.numpy(), rtol=1e-7, atol=1e-8 * (1.0 + float(gz.abs().max())))
    e = t.engine.calls
    assert e["sgpmc_lik_rows"] == e["sgpmc_lik_tail"] == 6 and e["sgpmc_tail"] == 0 and e["t_handed_over"] == 3
    assert t.last_pass1 == "sgpmc_lik_rows"


def test_gaussian_keeps_the_existing_path_and_numbers():
    import sgpmc_reference as R0
    X, y, Z = problem("gaussian")
    eng = SgpmcLikOracleEngine()
    t0 = ggp_amd.SgpmcTarget(X, y, Z, jitter=JITTER, engine=eng)
    t1 = ggp_amd.SgpmcTarget(X, y, Z, jitter=JITTER, engine=eng, likelihood="gaussian")
    q = np.asarray(t0.start()) + 0.2 * np.random.default_rng(1).standard_normal(t0.ndim)
    a, b = t0.logp_and_grad(q), t1.logp_and_grad(q)
    assert t1.ndim == 2 + 2 + 6 and a[0] == b[0] and a[1] == b[1]
    assert eng.calls["sgpmc_lik_rows"] == 0 and eng.calls["sgpmc_tail"] == 2
    assert abs(a[0] - float(R0.logp_torch(torch.as_tensor(q), X, y, Z, JITTER))) <= 1e-10 * (1.0 + abs(a[0]))


def test_bad_labels_counts_and_names_raise():
    X, y, Z = problem("poisson")
    eng = SgpmcLikOracleEngine()
    mk = lambda yy, lik: ggp_amd.SgpmcTarget(X, torch.as_tensor(yy), Z, engine=eng, likelihood=lik)
    n = X.shape[0]
    for bad in (np.full(n, 0.5), np.full(n, -1.0), np.r_[np.nan, np.ones(n - 1)]):
        with pytest.raises(ValueError):
            mk(bad, "poisson")
    for lik in ("bernoulli", "bernoulli_logit"):
        for bad in (np.full(n, 2.0), np.r_[0.0, -np.ones(n - 1)], np.full(n, 0.5)):
            with pytest.raises(ValueError):
                mk(bad, lik)
        assert bool((mk(np.r_[0.0, np.ones(n - 1)], lik).y == torch.as_tensor(np.r_[-1.0, np.ones(n - 1)])).all())
    with pytest.raises(ValueError):
        mk(np.ones(n), "softmax")
    from ggp_amd.gp_shim import BernoulliLikelihood, PoissonLikelihood
    assert BernoulliLikelihood().name == "bernoulli" and BernoulliLikelihood(link="logit").name == "bernoulli_logit"
    assert PoissonLikelihood().name == "poisson" and not hasattr(PoissonLikelihood(), "noise") and not hasattr(BernoulliLikelihood("logit"), "noise")
    with pytest.raises(ValueError):
        BernoulliLikelihood(link="cauchit")
    Xt = torch.rand(8, 1, dtype=torch.float64)
    with pytest.raises(ValueError):
        ggp_amd.BayesianStochasticVariationalGP(Xt, torch.ones(8, dtype=torch.float64), PoissonLikelihood(), Xt[:3].clone(), engine=eng)


@pytest.mark.parametrize("lik", NEW)
def test_predictive_moments_against_direct_sampling(lik):
    """E y and sd y of ``likelihood_moments`` against n = 4e5 direct draws of f and y.  The bound is 6 standard errors of the two
    estimators: sd / sqrt(n) for the mean, and for the standard deviation sqrt(m4 - sd^4) / (2 sd sqrt(n)) with the sample's own
    fourth central moment."""
    rng = np.random.default_rng(12)
    n = 400_000
    for mu, var in ((0.3, 0.5), (-1.2, 0.1), (1.0, 1.5)):
        f = mu + math.sqrt(var) * rng.standard_normal(n)
        if lik == "poisson":
            ys = rng.poisson(np.exp(f)).astype(np.float64)
        else:
            p = 0.5 * (1.0 + np.vectorize(math.erf)(f / math.sqrt(2.0))) if lik == "bernoulli" else 1.0 / (1.0 + np.exp(-f))
            ys = (rng.uniform(size=n) < p).astype(np.float64)
        m, s = likelihood_moments(lik, np.array([mu]), np.array([var]))
        sd = ys.std()
        m4 = ((ys - ys.mean()) ** 4).mean()
        assert abs(m[0] - ys.mean()) <= 6.0 * sd / math.sqrt(n)
        assert abs(s[0] - sd) <= 6.0 * math.sqrt(max(m4 - sd ** 4, 0.0)) / (2.0 * sd * math.sqrt(n))


def test_predict_sgpmc_returns_the_moments_of_y():
    lik = "poisson"
    X, y, Z = problem(lik)
    eng = SgpmcLikOracleEngine()
    model, trace, _ = ggp_amd.train_sgp_hmc((X, y), Z, 2, tune=3, num_samples=4, engine=eng, seed=2, warmup_iters=3, likelihood=lik)
    assert model.likelihood == lik and len(trace) == 4 and "noise_variance" not in trace[0]
    Xs = torch.as_tensor(np.random.default_rng(0).uniform(-2, 2, (5, 2)))
    pm, ym, ys = ggp_amd.predict_sgpmc(model, trace, Xs)
    assert pm.shape == (5,) and ym.shape == ys.shape == (4, 5) and np.allclose(pm, ym.mean(0))
    row = trace[0]
    mean, var, _ = eng.svgp_predict(Xs, model.Z, list(row["lengthscales"]), float(row["variance"]), torch.as_tensor(row["V"]),
                                    torch.zeros(6, 6, dtype=torch.float64), jitter=model.jitter)
    m = np.exp(mean.numpy() + 0.5 * var.numpy())
    assert np.allclose(ym[0], m) and np.allclose(ys[0], np.sqrt(m + np.expm1(var.numpy()) * m * m)) and (ys > 0).all()


def test_bad_arguments_are_rejected_before_any_launch():
    """SGP_ERR_ARG before SGP_ERR_DIM before SGP_ERR_WORKSPACE, on dummy pointers that are never dereferenced."""
    import __graft_entry__ as ge
    ge.build()
    lib = ggp_amd.load_library()
    one, null = C.c_void_p(8), C.c_void_p(0)
    big = 1 << 40
    inv = (C.c_double * 2)(1.0, 1.0)

    def rows(X=one, ldx=2, y=one, Z=one, ldz=2, inv_ls=inv, sf2=1.0, s2=1.0, v=one, N=10, M=4, d=2, kid=0, lik=3, linv=one, adj=1, out=one,
             G=one, g=one, dmu=one, dv=one, T=one, ws=null, nbytes=0):
        return lib.sgp_sgpmc_lik_rows(X, ldx, y, Z, ldz, inv_ls, sf2, s2, v, N, M, d, kid, lik, linv, adj, out, G, g, dmu, dv, T, ws, nbytes, null)

    for name in ("X", "y", "Z", "v", "linv", "out", "G", "g", "dmu", "dv", "T"):
        assert rows(**{name: null}) == -1, name
    assert rows(inv_ls=None) == -1 and rows(ldx=1) == -1 and rows(ldz=1) == -1 and rows(N=-1) == -1 and rows(M=0) == -1 and rows(d=0) == -1
    assert rows(kid=3) == -1 and rows(kid=-1) == -1 and rows(kid=4) == -1                       # composite: not here
    assert rows(lik=-1) == -1 and rows(lik=4) == -1
    assert rows(lik=0, s2=0.0) == -1 and rows(lik=0, s2=-1.0) == -1 and rows(lik=0, s2=float("nan")) == -1
    assert rows(lik=1, s2=0.0) == -3 and rows(lik=2, s2=-1.0) == -3                             # s2 is the Gaussian's alone
    assert rows(M=4097) == -2 and rows(d=33, ldx=33, ldz=33) == -2 and rows(M=4097, T=null) == -1
    assert rows() == -3 and rows(ws=one, nbytes=1) == -3 and rows(ws=null, nbytes=big) == -3
    assert rows(adj=0, G=null, g=null) == -3                                                    # valid without the adjoints, but for its workspace
    q = lib.sgp_sgpmc_lik_rows_workspace_bytes
    assert q(10, 4, 33) == 0 and q(10, 4097, 2) == 0 and q(-1, 4, 2) == 0 and 0 < q(10, 4, 2) < q(100000, 256, 2)
    # a shard that does not fit one super-chunk of K'_fu: no size, and the call says SGP_ERR_WORKSPACE
    lib.sgp_set_kfu_budget_bytes(1 << 20)
    try:
        assert q(4096, 128, 2) == 0 and rows(N=4096, M=128, ws=one, nbytes=big) == -3 and q(1024, 128, 2) > 0
    finally:
        lib.sgp_set_kfu_budget_bytes(0)

    def tail(r=one, G=one, g=one, v=one, N=10, M=4, adj=1, out=one, vbar=one, bbar=one, Kuubar=one, linv=one, ws=null, nbytes=0):
        return lib.sgp_sgpmc_lik_tail(r, G, g, v, N, M, adj, out, vbar, bbar, Kuubar, linv, ws, nbytes, null)

    for name in ("r", "G", "g", "v", "out", "vbar", "bbar", "Kuubar", "linv"):
        assert tail(**{name: null}) == -1, name
    assert tail(M=0) == -1 and tail(N=-1) == -1 and tail(M=4097) == -2 and tail(M=4097, v=null) == -1
    assert tail() == -3 and tail(ws=one, nbytes=1) == -3
    assert tail(adj=0, G=null, g=null, vbar=null, bbar=null, Kuubar=null, linv=null) == -3
    assert lib.sgp_sgpmc_lik_workspace_bytes(0) == 0 and 0 < lib.sgp_sgpmc_lik_workspace_bytes(128) < lib.sgp_sgpmc_lik_workspace_bytes(129)
