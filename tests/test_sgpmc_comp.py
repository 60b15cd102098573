"""CPU: ``composite.CompositeSgpmcTarget``, ``sample_hmc`` and the model functions of ``sgp_hmc`` over the CPU double
tests/sgpmc_comp_double.py; the argument checks of sgp_sgpmc_comp_rows / sgp_sgpmc_comp_bwd through the C ABI (no launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ggp_amd
import sgpmc_comp_reference as R
from sgpmc_comp_double import SgpmcCompOracleEngine
from sgpmc_double import SgpmcOracleEngine

T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def problem(N=40, M=6, d=1, seed=0, lik="gaussian"):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(0.0, 6.0, (N, d)), 0)
    f = np.sin(X.sum(1)) + 0.3 * X[:, 0]
    y = rng.poisson(np.exp(f)).astype(np.float64) if lik == "poisson" else f + 0.1 * rng.standard_normal(N)
    return X, y, X[rng.permutation(N)[:M]].copy()


def co2_target(X, y, Z, lik="gaussian", priors="co2", **kw):
    white, mean = kw.pop("white", 1.0), kw.pop("mean", "linear")
    if priors == "co2":     # the reference's priors on what this target samples
        drop = ([] if lik == "gaussian" else ["noise_variance"]) + ([] if white else ["white"]) + ([] if mean else ["mean_A", "mean_b"])
        priors = {k: v for k, v in ggp_amd.CO2_SGPMC_PRIORS.items() if k not in drop}
    return ggp_amd.CompositeSgpmcTarget(T(X), T(y), T(Z), ggp_amd.co2_sgpmc_kernel(), priors=priors, white=white, mean=mean,
                                        likelihood=lik, engine=SgpmcCompOracleEngine(), **kw)


def test_names_start_and_constrain():
    X, y, Z = problem(d=2)
    t = co2_target(X, y, Z)
    assert t.names == ["variance_0", "lengthscale_0_0", "lengthscale_0_1", "variance_1", "lengthscale_1_0", "alpha_1_0", "variance_2",
                       "lengthscale_2_0", "variance_3", "lengthscale_3_0", "white", "noise_variance", "mean_A", "mean_A", "mean_b"]
    assert t.ndim == 15 + 6 and set(ggp_amd.CO2_SGPMC_PRIORS) == set(t.names)
    c = t.constrain(t.start())
    for name in t.names[:12]:       # GPflow's defaults: 1 everywhere but the trend's variance log(2)^2
        assert c[name] == pytest.approx(math.log(2.0) ** 2 if name == "variance_2" else 1.0, rel=1e-12), name
    assert np.array_equal(c["mean_A"], [1.0, 1.0]) and c["mean_b"] == 0.0 and not c["V"].any()
    assert c["kernel"].block() == pytest.approx(ggp_amd.co2_sgpmc_kernel().block(), rel=1e-12)
    assert "period_0_0" not in t.names     # the period is fixed (co2_sgpmc.py:72)
    assert co2_target(X, np.round(np.abs(y)), Z, lik="poisson", white=None, mean=None).names == t.names[:10]
    with pytest.raises(ValueError, match="does not sample"):
        co2_target(X, y, Z, priors={"variance_7": ("gamma", 2.0, 1.0)})
    with pytest.raises(ValueError, match="unknown prior"):
        co2_target(X, y, Z, priors={"white": ("beta", 2.0, 1.0)})


@pytest.mark.parametrize("lik", ["gaussian", "poisson", "bernoulli"])
def test_target_gradient_against_central_differences(lik):
    """Every parameter kind present: variances, lengthscales, alpha, white, the likelihood variance (Gaussian), A, b and V."""
    X, y, Z = problem(lik=lik)
    if lik == "bernoulli":
        y = (y > np.median(y)).astype(np.float64)
    t = co2_target(X, y, Z, lik=lik)
    q = np.asarray(t.start()) + 0.3 * np.random.default_rng(1).standard_normal(t.ndim)
    lp, g = t.logp_and_grad(q)
    assert lp == t.logp(q) and len(g) == t.ndim
    h = 1e-6
    fd = np.array([(t.logp(q + h * e) - t.logp(q - h * e)) / (2 * h) for e in np.eye(t.ndim)])
    # central differences of a float64 logp: h^2 logp''' + eps |logp| / h ~ 1e-7 of |logp| + max|g|
    assert np.abs(fd - np.asarray(g)).max() <= 1e-7 * (abs(lp) + np.abs(g).max()), np.abs(fd - np.asarray(g)).max()


def test_prior_terms_against_scipy_and_the_log_jacobian():
    """logp = F (the long-double reference's) + sum of the scipy.stats log densities at the constrained values + log sigmoid(x) of
    every positive entry; a name without a prior contributes its Jacobian alone."""
    from scipy import stats
    X, y, Z = problem(d=2)
    t = co2_target(X, y, Z)
    q = np.asarray(t.start()) + 0.3 * np.random.default_rng(2).standard_normal(t.ndim)
    block, white, s2, A, b, cons = t.unpack(q)
    F = float(R.reference(X, y, Z, block, white, s2, A, b, 1e-4, "gaussian", q[t.n_theta:], grads=False)[0]["F"])
    dist = {"gamma": lambda a, r: stats.gamma(a, scale=1.0 / r), "halfnormal": lambda s: stats.halfnorm(scale=s),
            "normal": lambda m, s: stats.norm(m, s)}
    lp_prior = sum(dist[ggp_amd.CO2_SGPMC_PRIORS[n][0]](*ggp_amd.CO2_SGPMC_PRIORS[n][1:]).logpdf(c) for n, c in zip(t.names, cons))
    jac = sum(-np.logaddexp(0.0, -x) for n, x in zip(t.names, q) if n not in ("mean_A", "mean_b"))
    assert t.logp(q) == pytest.approx(F + lp_prior + jac, abs=1e-9 * (1.0 + abs(F)))
    bare = co2_target(X, y, Z, priors=None)
    assert bare.logp(q) == pytest.approx(F + jac, abs=1e-9 * (1.0 + abs(F)))


def test_one_term_expquad_equals_the_rbf_sgpmc_target():
    """d = 1, no white, no mean, Gamma(2, 1) priors, jitter 1e-5: q = [variance | lengthscale | noise | V] in both classes.  The
    tolerances of the existing target tests: logp to 1e-8 N, the gradient to 1e-6 max|g|.  This carries the exact-posterior pin of
    ``SgpmcTarget`` over to the new class."""
    from test_sgpmc_comp_gpu import one_term_pair
    X, y, Z = problem(N=60, M=7, seed=3)
    a, b = one_term_pair(X, y, Z, SgpmcCompOracleEngine(), SgpmcOracleEngine(), T)
    assert a.names == ["variance_0", "lengthscale_0_0", "noise_variance"] and a.ndim == b.ndim
    rng = np.random.default_rng(4)
    for _ in range(3):
        q = np.asarray(b.start()) + np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.standard_normal(7)])
        (la, ga), (lb, gb) = a.logp_and_grad(q), b.logp_and_grad(q)
        assert abs(la - lb) <= 1e-8 * 60, (la, lb)
        assert np.abs(np.asarray(ga) - np.asarray(gb)).max() <= 1e-6 * np.abs(gb).max()


def test_failures_are_a_zero_density_never_an_exception():
    X, y, Z = problem()
    Zd = Z.copy()
    Zd[1] = Zd[0]     # a duplicated inducing input without jitter and without white: K_uu is singular
    bad = co2_target(X, y, Zd, white=None, jitter=0.0)
    lp, g = bad.logp_and_grad(bad.start())
    assert lp == -math.inf and g == [0.0] * bad.ndim and bad.logp(bad.start()) == -math.inf
    t = co2_target(X, y, Z)
    q = np.asarray(t.start())
    for v in (float("nan"), 800.0):
        qn = q.copy()
        qn[0] = v
        assert t.logp_and_grad(qn) == (-math.inf, [0.0] * t.ndim)
    with pytest.raises(ValueError, match="entries"):
        t.logp(q[:-1])


def test_same_seed_same_chain_and_the_model_functions():
    X, y, Z = problem(N=30, M=5)
    kw = dict(priors=ggp_amd.CO2_SGPMC_PRIORS, seed=7, num_leapfrog_steps=3)
    model, a, secs = ggp_amd.train_sgp_hmc_composite((X, y), Z, ggp_amd.co2_sgpmc_kernel(), 2, 4, engine=SgpmcCompOracleEngine(), **kw)
    _, b, _ = ggp_amd.train_sgp_hmc_composite((X, y), Z, ggp_amd.co2_sgpmc_kernel(), 2, 4, engine=SgpmcCompOracleEngine(), **kw)
    assert isinstance(model, ggp_amd.CompositeSgpmcModel) and model.jitter == 1e-4 and len(a) == 4 and secs > 0.0
    assert np.array_equal(a["theta_unc"], b["theta_unc"]) and np.array_equal(a.get_sampler_stats("is_accepted"), b.get_sampler_stats("is_accepted"))
    assert a["variance_0"].shape == (4,) and a["mean_A"].shape == (4, 1) and a["V"].shape == (4, 5)
    assert model.target.engine.calls["sgpmc_comp_rows"] == model.target.n_evals > 0
    # the predictive: shapes, and the mean function's shift
    Xs = np.linspace(-0.5, 6.5, 9)[:, None]
    pm, fm, ys = ggp_amd.predict_sgpmc(model, a, Xs)
    assert pm.shape == (9,) and fm.shape == ys.shape == (4, 9) and (ys > 0).all() and np.allclose(pm, fm.mean(0))
    shifted = []
    for row in a:
        q = np.array(row["theta_unc"])
        q[model.target.names.index("mean_b")] += 0.75
        q[model.target.names.index("mean_A")] += 0.5
        shifted.append({"theta_unc": q})
    pm2, fm2, ys2 = ggp_amd.predict_sgpmc(model, ggp_amd.Trace(shifted, {}, varnames=()), Xs)
    assert np.allclose(fm2 - fm, 0.75 + 0.5 * Xs[:, 0], rtol=0, atol=1e-12) and np.array_equal(ys2, ys)


def test_bad_arguments_are_rejected_before_any_launch():
    """SGP_ERR_ARG before SGP_ERR_DIM before SGP_ERR_WORKSPACE, on dummy pointers that are never dereferenced."""
    import __graft_entry__ as ge
    ge.build()
    lib = ggp_amd.load_library()
    one, null = C.c_void_p(8), C.c_void_p(0)
    big = 1 << 40
    blk = (C.c_double * 33)(*ggp_amd.co2_sgpmc_kernel().block())

    def rows(X=one, ldx=2, y=one, mean=null, Z=one, ldz=2, block=blk, white=0.1, s2=0.1, v=one, N=10, M=4, d=2, lik=0, linv=one, adj=1,
             out=one, G=one, g=one, dmu=one, dv=one, mu=null, var=null, t=one, ws=null, nbytes=0):
        return lib.sgp_sgpmc_comp_rows(X, ldx, y, mean, Z, ldz, block, white, s2, v, N, M, d, lik, linv, adj, out, G, g, dmu, dv, mu, var, t,
                                       ws, nbytes, null)

    for name in ("X", "Z", "v", "linv", "out", "G", "g", "dmu", "dv", "t"):
        assert rows(**{name: null}) == -1, name
    assert rows(block=None) == -1 and rows(ldx=1) == -1 and rows(ldz=1) == -1 and rows(N=-1) == -1 and rows(M=0) == -1 and rows(d=0) == -1
    assert rows(d=9, ldx=9, ldz=9) == -1                                                  # d > COMP_MAX_DIM
    for slot, val in ((0, 5.0), (0, 0.0), (1, -1.0), (2, 3.0), (3, 7.0), (4, 0.0), (5, 0.0)):   # a block comp_parse rejects
        b2 = (C.c_double * 33)(*ggp_amd.co2_sgpmc_kernel().block())
        b2[slot] = val
        assert rows(block=b2) == -1, (slot, val)
    assert rows(lik=-1) == -1 and rows(lik=4) == -1
    assert rows(s2=0.0) == -1 and rows(s2=-1.0) == -1 and rows(s2=float("nan")) == -1
    assert rows(lik=3, s2=0.0) == -3                                                      # s2 is the Gaussian's alone
    assert rows(white=-1e-3) == -1 and rows(white=float("nan")) == -1 and rows(white=0.0) == -3
    assert rows(y=null) == -1 and rows(y=null, adj=0, dmu=null, dv=null) == -3            # moments only: no adjoints, no dmu / dv
    assert rows(M=4097) == -2 and rows(M=4097, t=null) == -1 and rows(M=4097, ws=one, nbytes=big) == -2
    assert rows() == -3 and rows(ws=one, nbytes=1) == -3 and rows(ws=null, nbytes=big) == -3
    assert rows(adj=0, G=null, g=null) == -3 and rows(N=0, X=null, y=null, dmu=null, dv=null) == -3
    q = lib.sgp_sgpmc_comp_rows_workspace_bytes
    assert q(10, 4, 9) == 0 and q(10, 4097, 2) == 0 and q(-1, 4, 2) == 0 and q(10, 0, 2) == 0 and 0 < q(0, 4, 2) <= q(10, 4, 2) < q(100000, 256, 2)
    assert q(1 << 20, 128, 1) - q(65536, 128, 1) < 64 << 20     # K_fu is one COMP_CHUNK_ROWS chunk (64 MiB here) whatever N is

    def bwd(X=one, ldx=2, dmu=one, Z=one, ldz=2, block=blk, t=one, linv=one, bbar=one, N=10, M=4, d=2, g=one, ws=null, nbytes=0):
        return lib.sgp_sgpmc_comp_bwd(X, ldx, dmu, Z, ldz, block, t, linv, bbar, N, M, d, g, ws, nbytes, null)

    for name in ("X", "dmu", "Z", "t", "linv", "bbar", "g"):
        assert bwd(**{name: null}) == -1, name
    assert bwd(block=None) == -1 and bwd(ldx=1) == -1 and bwd(ldz=1) == -1 and bwd(N=-1) == -1 and bwd(M=0) == -1 and bwd(d=9, ldx=9, ldz=9) == -1
    assert bwd(M=4097) == -2 and bwd(M=4097, g=null) == -1
    assert bwd() == -3 and bwd(ws=one, nbytes=1) == -3 and bwd(ws=null, nbytes=big) == -3
    qb = lib.sgp_sgpmc_comp_bwd_workspace_bytes
    assert qb(10, 4, 9) == 0 and qb(10, 4097, 2) == 0 and qb(-1, 4, 2) == 0 and 0 < qb(10, 4, 2) < qb(100000, 256, 2)


def test_the_three_existing_refusals_still_hold():
    import __graft_entry__ as ge
    ge.build()
    lib = ggp_amd.load_library()
    X, y, Z = problem()
    with pytest.raises(ValueError, match="composite kernels are not supported"):
        ggp_amd.SgpmcTarget(T(X), T(y), T(Z), kernel="composite", engine=SgpmcOracleEngine())
    one, null, inv = C.c_void_p(8), C.c_void_p(0), (C.c_double * 33)(*ggp_amd.co2_sgpmc_kernel().block())
    assert lib.sgp_sgpmc_lik_rows(one, 2, one, one, 2, inv, 1.0, 0.1, one, 10, 4, 2, 3, 0, one, 1, one, one, one, one, one, one, one, 1 << 40,
                                  null) == -1
    assert lib.sgp_suffstats_bwd_factored_ex(one, 2, one, one, 2, inv, 1.0, one, one, 0.1, one, 0.0, 10, 4, 2, 3, one, one, one, null, one,
                                             1 << 40, null) == -1
