"""CPU: the SGPMC density and its adjoints (tests/sgpmc_reference.py), ``targets.SgpmcTarget`` / ``hmc.sample_hmc`` / ``sgp_hmc`` over
the CPU double (tests/sgpmc_double.py), and the sampler against an EXACT posterior (tests/golden/posterior_sgpmc_d1_tiny.npz)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

import ggp_amd
import pass2_reference as P2
import sgpmc_reference as R
from oracle import vfe_oracle as O
from sgpmc_double import SgpmcOracleEngine
from test_posterior_pin import ess

T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
JITTER = 1e-5


def small_problem(seed=0, N=40, M=7, d=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    Z = X[rng.choice(N, M, replace=False)] + 0.05 * rng.standard_normal((M, d))
    return X, y, Z, np.array([0.9, 1.4])[:d], 1.3, 0.2, rng.standard_normal(M)


def tail_torch(K, Phi, b, yy, kappa, v, s2, N):
    """F as a torch fp64 function of the explicit K, Phi, b: autograd delivers the adjoints the tail hands to pass 2 / sgp_kuu_bwd."""
    M = K.shape[0]
    L = torch.linalg.cholesky(K)
    t = torch.linalg.solve_triangular(L.T, v[:, None], upper=True)[:, 0]
    Li = torch.linalg.solve_triangular(L, torch.eye(M, dtype=torch.float64), upper=False)
    Q = yy - 2.0 * (t @ b) + t @ Phi @ t + kappa - ((Li @ Phi) * Li).sum()
    return -0.5 * N * torch.log(2.0 * math.pi * s2) - Q / (2.0 * s2) - 0.5 * (v @ v) - 0.5 * M * math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------
# 1 / 2. the long-double reference, autograd, and the Cholesky-adjoint term
# ---------------------------------------------------------------------------------------------
def test_long_double_reference_agrees_with_autograd():
    """Every output of the long-double reference against torch autograd of the same scalar in fp64, |got - ref| <= 1e-12 A: the bound
    of tests/test_pass2_kernel.py (4500 unit round-offs of the condition scale, for sums of M ~ 10 terms behind a substitution)."""
    X, y, Z, ls, sf2, s2, v = small_problem()
    K, Phi, b, yy, kappa = R.kernel_blocks(X, y, Z, ls, sf2, JITTER, 0)
    ref, A = R.reference(K, Phi, b, yy, kappa, v, s2, X.shape[0])
    f64 = lambda a: T(np.asarray(a, dtype=np.float64))
    Kt, Pt, bt, vt = (f64(a).requires_grad_(True) for a in (K, Phi, b, v))
    s2t, kt = torch.tensor(s2, dtype=torch.float64, requires_grad=True), torch.tensor(float(kappa), dtype=torch.float64, requires_grad=True)
    F = tail_torch(Kt, Pt, bt, float(yy), kt, vt, s2t, X.shape[0])
    F.backward()
    Li = ref["Linv"]
    worst = {"F": P2.assert_close(F.detach().numpy(), ref["F"], A["F"], what="F"),
             "vbar": P2.assert_close(vt.grad.numpy(), ref["vbar"], A["vbar"], what="vbar"),
             "s2bar": P2.assert_close(s2t.grad.numpy(), ref["s2bar"], A["s2bar"], what="s2bar"),
             "kappabar": P2.assert_close(kt.grad.numpy(), ref["kappabar"], A["kappabar"], what="kappabar"),
             "bbar": P2.assert_close(bt.grad.numpy(), ref["bbar"], A["bbar"], what="bbar"),
             # 2 s2 Phibar = L^-T Cw L^-1
             "Phibar": P2.assert_close(Pt.grad.numpy(), Li.T @ ref["Cw"] @ Li / (2 * R.LD(s2)),
                                       np.abs(Li).T @ A["Cw"] @ np.abs(Li) / (2 * R.LD(s2)), what="Phibar from Cw"),
             "Kuubar": P2.assert_close(0.5 * (Kt.grad + Kt.grad.T).numpy(), ref["Kuubar"], A["Kuubar"], what="Kuubar")}
    print(worst)
    # the two statements of F agree too: the torch restatement in GPflow's op order (A = L^-1 K_uf) against the long double
    F2 = R.density_torch(v, X, y, Z, ls, sf2, s2, JITTER, 0)
    P2.assert_close(F2.numpy(), ref["F"], A["F"], what="density_torch")


def dF_dZ_entries(X, y, Z, ls, sf2, s2, v, low_mode, entries):
    """(analytic dF/dZ from the long-double adjoints through the long-double pass 2 and K_uu gradient, central differences of the
    long-double F) at the given (m, j) entries."""
    ref, _ = R.reference_at(X, y, Z, ls, sf2, s2, JITTER, 0, v, low_mode)
    g1, _ = P2.bwd_factored_reference(X, y, Z, ls, sf2, ref["Linv"], ref["Cw"], s2, ref["bbar"], ref["kappabar"], 0)
    g2, _ = P2.kuu_bwd_reference(Z, ls, sf2, ref["Kuubar"], 0)
    gz = g1["Z"] + g2["Z"]
    step = R.LD(1e-5)
    fd = []
    for m, j in entries:
        vals = []
        for sgn in (1, -1):
            Zp = P2._ld(Z).copy()
            Zp[m, j] += sgn * step
            K, Phi, b, yy, kappa = R.kernel_blocks(X, y, Zp, ls, sf2, JITTER, 0)   # (Zp stays long double: _ld keeps what it is given)
            vals.append(R.reference(K, Phi, b, yy, kappa, v, s2, X.shape[0])[0]["F"])
        fd.append((vals[0] - vals[1]) / (2 * step))
    return np.array([gz[m, j] for m, j in entries], R.LD), np.array(fd, R.LD), float(np.abs(gz).max())


ENTRIES = [(0, 0), (2, 1), (3, 0), (5, 1), (6, 0)]
# central differences with step 1e-5 in long double: truncation ~ step^2 x (third derivative / first) ~ 1e-10 relative, cancellation
# 1.1e-19 x A_F / step ~ 1e-11 absolute against gradients of order 10: 1e-8 of the largest entry leaves two decades
FD_RTOL = 1e-8


def test_cholesky_adjoint_term_of_kuubar_through_dF_dZ():
    X, y, Z, ls, sf2, s2, v = small_problem()
    an, fd, scale = dF_dZ_entries(X, y, Z, ls, sf2, s2, v, "ok", ENTRIES)
    err = float(np.abs(an - fd).max()) / scale
    print("dF/dZ analytic vs central differences: %.3e of the largest entry" % err)
    assert err <= FD_RTOL, (an, fd)


@pytest.mark.parametrize("low_mode", ["dropped", "transposed"])
def test_the_dF_dZ_comparison_fails_without_the_right_cholesky_adjoint(low_mode):
    """The same comparison with the low() term dropped, or applied as the upper triangle: off by many decades more than FD_RTOL."""
    X, y, Z, ls, sf2, s2, v = small_problem()
    an, fd, scale = dF_dZ_entries(X, y, Z, ls, sf2, s2, v, low_mode, ENTRIES)
    err = float(np.abs(an - fd).max()) / scale
    print("low() %s: %.3e" % (low_mode, err))
    assert err > 1e4 * FD_RTOL


# ---------------------------------------------------------------------------------------------
# 3. Gaussian in v: the mode and the marginal identity against the oracle's collapsed bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rbf_d3_small", "m52_d3_small"])
def test_gaussian_in_v_identities_against_the_collapsed_bound(name):
    G = load_golden(name)
    X, y, Z, ls = T(G["X"]), T(G["y"]), T(G["Z"]), T(G["ls"])
    sf2, s2, kid = float(G["sf2"]), float(G["s2"]), int(G["kernel_id"])
    N, M = X.shape[0], Z.shape[0]
    e = SgpmcOracleEngine()
    Kuu = O.kuu(Z, ls, sf2, JITTER, kid)
    L = torch.linalg.cholesky(Kuu)
    linv, _ = e.kuu_factor(Kuu)
    st = O.suffstats_whitened(X, y, Z, ls, sf2, L, kid)
    packed = torch.cat([st.Phi.reshape(-1), st.b, torch.tensor([st.yy, st.kappa], dtype=torch.float64)])
    B = torch.eye(M, dtype=torch.float64) + st.Phi / s2
    m = torch.linalg.solve(B, st.b) / s2
    res = e.sgpmc_tail(packed, m, s2, N, linv, with_adjoints=True)
    vfe = float(O.vfe_pymc3_order(X, y, Z, ls, math.sqrt(sf2), math.sqrt(s2), jitter=JITTER, kernel_id=kid))
    marg = float(res["out"][0]) + 0.5 * M * math.log(2.0 * math.pi) - 0.5 * float(torch.linalg.slogdet(B)[1])
    print(name, "marginal identity %.3e per datum, |grad_v F(m)| max %.3e" % (abs(marg - vfe) / N, float(res["vbar"].abs().max())))
    assert abs(marg - vfe) <= 1e-8 * N
    assert float(res["vbar"].abs().max()) <= 1e-8 * N
    # -d2F/dv2 = B: the gradient is linear in v with slope -B
    dv = torch.linspace(-1.0, 1.0, M, dtype=torch.float64)
    res2 = e.sgpmc_tail(packed, m + dv, s2, N, linv, with_adjoints=True)
    assert float((res2["vbar"] - res["vbar"] + B @ dv).abs().max()) <= 1e-8 * N


# ---------------------------------------------------------------------------------------------
# 4. SgpmcTarget over the double
# ---------------------------------------------------------------------------------------------
def target_and_point(seed=1):
    G = load_golden("rbf_d3_small")
    X, y, Z = T(G["X"]), T(G["y"]), T(G["Z"])
    tgt = ggp_amd.SgpmcTarget(X, y, Z, engine=SgpmcOracleEngine())
    q = np.asarray(tgt.start()) + np.random.default_rng(seed).uniform(-0.4, 0.4, tgt.ndim)
    return tgt, q, X, y, Z


def test_target_matches_autograd_of_the_restatement():
    tgt, q, X, y, Z = target_and_point()
    assert tgt.ndim == 3 + 2 + 30 and tgt.jitter == 1e-5
    lp, g, gz = tgt.logp_and_grad(q, want_gz=True)
    lp2, g2 = tgt.logp_and_grad(q)
    assert lp2 == lp and g2 == g and tgt.logp(q) == pytest.approx(lp, abs=1e-9)
    assert tgt.last_pass1 == "suffstats_whitened" and tgt.engine.calls["sgpmc_tail"] == 3 and tgt.engine.calls["suffstats_bwd_factored"] == 2
    qt, Zt = T(q).requires_grad_(True), Z.clone().requires_grad_(True)
    ref = R.logp_torch(qt, X, y, Zt, JITTER, 0)
    ref.backward()
    N = X.shape[0]
    assert abs(lp - float(ref.detach())) <= 1e-8 * N
    gr = qt.grad.numpy()
    assert np.abs(np.asarray(g) - gr).max() <= 1e-6 * np.abs(gr).max()
    assert float((gz - Zt.grad).abs().max()) <= 1e-6 * float(Zt.grad.abs().max())
    # the streaming layout of the whitened pass 1, T handed to pass 2
    tgt.whitened_rows_min_work = 0
    lp3, g3 = tgt.logp_and_grad(q)
    assert tgt.last_pass1 == "suffstats_whitened_rows" and tgt.engine.calls["t_handed_over"] == 1
    assert abs(lp3 - lp) <= 1e-8 * N and np.abs(np.asarray(g3) - gr).max() <= 1e-6 * np.abs(gr).max()
    c = tgt.constrain(q)
    assert set(c) == {"variance", "lengthscales", "noise_variance", "V"} and len(c["lengthscales"]) == 3 and c["V"].shape == (30,)


def test_target_start_and_refusals():
    tgt, q, X, y, Z = target_and_point()
    c = tgt.constrain(tgt.start())
    assert c["variance"] == pytest.approx(math.log(2.0) ** 2, rel=1e-12) and c["noise_variance"] == pytest.approx(1.0, rel=1e-12)
    assert np.allclose(c["lengthscales"], math.log(2.0), rtol=1e-12) and not c["V"].any()
    with pytest.raises(ValueError, match="composite"):
        ggp_amd.SgpmcTarget(X, y, Z, kernel="composite", engine=SgpmcOracleEngine())
    # a duplicated inducing input without jitter: K_uu is singular, the density is zero there -- never an exception
    Zd = Z.clone()
    Zd[1] = Zd[0]
    bad = ggp_amd.SgpmcTarget(X, y, Zd, jitter=0.0, engine=SgpmcOracleEngine())
    lp, g = bad.logp_and_grad(q)
    assert lp == -math.inf and g == [0.0] * bad.ndim and bad.logp(q) == -math.inf
    qn = q.copy()
    qn[0] = float("nan")
    assert tgt.logp_and_grad(qn) == (-math.inf, [0.0] * tgt.ndim)


def test_more_than_one_rank_is_refused(monkeypatch):
    import ggp_amd.core as core
    monkeypatch.setattr(core, "_world", lambda group: 2)
    G = load_golden("rbf_d1_tiny")
    with pytest.raises(ValueError, match="one process"):
        ggp_amd.SgpmcTarget(T(G["X"]), T(G["y"]), T(G["Z"]), engine=SgpmcOracleEngine(), group=object())


# ---------------------------------------------------------------------------------------------
# 5. sample_hmc on a standard normal
# ---------------------------------------------------------------------------------------------
class StdNormal:
    ndim = 5

    def start(self):
        return [0.0] * self.ndim

    def constrain(self, q):
        return {"x": np.asarray(q, dtype=np.float64).copy()}

    def logp_and_grad(self, q):
        q = np.asarray(q, dtype=np.float64)
        return -0.5 * float(q @ q), (-q).tolist()


def test_sample_hmc_step_rule_seed_and_moments():
    tr = ggp_amd.sample_hmc(StdNormal(), 40, 0, seed=3, num_adaptation_steps=25, step_size=0.05)
    eps, lr, acc = (np.asarray(tr.get_sampler_stats(k)) for k in ("step_size", "log_accept_ratio", "is_accepted"))
    assert tr.stat_names == {"is_accepted", "log_accept_ratio", "step_size", "perf_counter_diff"} and eps[0] == 0.05
    for i in range(39):
        if i < 25:
            want = eps[i] * 1.1 if min(0.0, lr[i]) > math.log(0.8) else eps[i] / 1.1
            assert eps[i + 1] == want, (i, eps[i], eps[i + 1], lr[i])
        else:
            assert eps[i + 1] == eps[i]
    assert len(set(eps[:26])) > 5 and len(set(eps[25:])) == 1
    x = tr["x"]
    moved = np.any(x[1:] != x[:-1], axis=1)
    assert np.array_equal(moved, acc[1:]) and np.all(acc[lr >= 0.0])          # a move is an acceptance; a non-negative ratio always accepts
    tr2 = ggp_amd.sample_hmc(StdNormal(), 40, 0, seed=3, num_adaptation_steps=25, step_size=0.05)
    assert np.array_equal(tr2["x"], x) and np.array_equal(tr2.get_sampler_stats("log_accept_ratio"), lr)
    assert not np.array_equal(ggp_amd.sample_hmc(StdNormal(), 40, 0, seed=4, num_adaptation_steps=25, step_size=0.05)["x"], x)
    # moments: a long chain with the step adapted during the whole burn-in
    tr = ggp_amd.sample_hmc(StdNormal(), 3000, 300, seed=5, num_adaptation_steps=300, step_size=0.05)
    assert len(tr) == 3000 and len(set(np.asarray(tr.get_sampler_stats("step_size")))) == 1
    x = tr["x"]
    for k in range(5):
        n1, n2 = ess(x[:, k]), ess(x[:, k] ** 2)
        assert n1 > 100 and n2 > 100
        assert abs(x[:, k].mean()) < 4.0 * math.sqrt(1.0 / n1), (k, x[:, k].mean(), n1)
        assert abs((x[:, k] ** 2).mean() - 1.0) < 4.0 * math.sqrt(2.0 / n2), (k, (x[:, k] ** 2).mean(), n2)   # Var[x^2] = 2


def test_sample_hmc_rejects_a_non_finite_energy():
    class Walled(StdNormal):
        def logp_and_grad(self, q):
            q = np.asarray(q, dtype=np.float64)
            if q[0] > 0.5:
                return -math.inf, [0.0] * self.ndim
            return -0.5 * float(q @ q), (-q).tolist()

    tr = ggp_amd.sample_hmc(Walled(), 200, 0, seed=1, start=[0.0] * 5, step_size=0.3, num_adaptation_steps=0)
    lr, acc = np.asarray(tr.get_sampler_stats("log_accept_ratio")), np.asarray(tr.get_sampler_stats("is_accepted"))
    assert np.any(np.isneginf(lr)) and not np.any(acc[np.isneginf(lr)]) and np.all(tr["x"][:, 0] <= 0.5)


# ---------------------------------------------------------------------------------------------
# 6. the exact-posterior pin
# ---------------------------------------------------------------------------------------------
def test_fixture_is_the_quadrature_of_the_restatement():
    """Spot check of the stored numbers without redoing the 1.4 M-node rule, with the restatement itself: the stored density at the
    stated point is F(m) + M/2 log 2 pi - 1/2 log det B + priors there, and importance sampling of the three hyper-parameters from
    N(mean, 1.5^2 cov) with that marginal reproduces the stored evidence (weights average to 1) and mean."""
    P = load_golden("posterior_sgpmc_d1_tiny")
    X, y, Z, jit = T(P["X"]), T(P["y"]), T(P["Z"]), float(P["jitter"])
    M = Z.shape[0]

    def marginal(x):
        sp = torch.nn.functional.softplus
        xt = T(x)
        sf2, ls, s2 = sp(xt[0]), sp(xt[1:2]), R.NOISE_FLOOR + sp(xt[2])
        K = O.kuu(Z, ls, float(sf2), jit, 0)
        A = torch.linalg.solve_triangular(torch.linalg.cholesky(K), O.kern(Z, X, ls, float(sf2), 0), upper=False)
        B = torch.eye(M, dtype=torch.float64) + A @ A.T / s2
        m = torch.linalg.solve(B, A @ y) / s2
        q = torch.cat([xt, m])
        return float(R.logp_torch(q, X, y, Z, jit, 0)) + 0.5 * M * math.log(2.0 * math.pi) - 0.5 * float(torch.linalg.slogdet(B)[1]), m.numpy()

    assert abs(marginal(P["x_spot"])[0] - float(P["logp_spot"])) < 1e-6
    rng = np.random.default_rng(1)
    Lc = np.linalg.cholesky(2.25 * P["cov"])
    z = rng.standard_normal((3000, 3))
    pts = P["mean"] + z @ Lc.T
    lq = -0.5 * (z * z).sum(1) - np.log(np.diag(Lc)).sum() - 1.5 * math.log(2 * math.pi)
    vals = [marginal(p) for p in pts]
    w = np.exp(np.array([v[0] for v in vals]) - lq - float(P["log_evidence"]))
    assert abs(w.mean() - 1.0) < 4.0 * w.std() / math.sqrt(w.size), (w.mean(), w.std())
    mean = (w[:, None] * pts).sum(0) / w.sum()
    assert np.all(np.abs(mean - P["mean"]) < 0.05 * np.sqrt(np.diag(P["cov"])) + 0.02), (mean, P["mean"])
    vm = (w[:, None] * np.array([v[1] for v in vals])).sum(0) / w.sum()
    assert np.all(np.abs(vm - P["v_mean"]) < 0.02 + 0.05 * np.sqrt(P["v_var"])), (vm, P["v_mean"])


# The stiffest direction of this posterior (v along the top eigenvector of B) has a standard deviation of ~0.02, the widest (x_var) 1.2:
# with the identity mass matrix the adapted step is ~0.02, and a trajectory must be ~90 steps long to cross the wide one.  63 000
# evaluations over the double: ~90 s here.
PIN_TUNE, PIN_DRAWS, PIN_LEAPFROG, PIN_SEED = 100, 600, 90, 23


def test_sample_hmc_reproduces_the_exact_posterior():
    """Means and variances of the three unconstrained hyper-parameters and E[v] within 4 MCSE of the quadrature; ESS > 100 for every
    pinned quantity or the test fails."""
    P = load_golden("posterior_sgpmc_d1_tiny")
    tgt = ggp_amd.SgpmcTarget(T(P["X"]), T(P["y"]), T(P["Z"]), jitter=float(P["jitter"]), engine=SgpmcOracleEngine())
    tr = ggp_amd.sample_hmc(tgt, PIN_DRAWS, PIN_TUNE, seed=PIN_SEED, num_adaptation_steps=PIN_TUNE, num_leapfrog_steps=PIN_LEAPFROG)
    eps = np.asarray(tr.get_sampler_stats("step_size"))
    assert len(set(eps)) == 1 and eps[0] != 0.01                      # adapted during the burn-in, frozen afterwards
    print("step %.4f, acceptance %.2f" % (eps[0], np.asarray(tr.get_sampler_stats("is_accepted")).mean()))
    q = tr["theta_unc"]
    mean, var, m4 = P["mean"], np.diag(P["cov"]), P["m4"]
    for k, name in enumerate(("x_var", "x_ls", "x_noise")):
        x = q[:, k]
        n_eff = ess(x)
        assert n_eff > 100, (name, n_eff)
        mcse = math.sqrt(var[k] / n_eff)
        assert abs(x.mean() - mean[k]) < 4.0 * mcse, "E[%s] = %.4f, exact %.4f, 4 MCSE = %.4f (ESS %.0f)" % (name, x.mean(), mean[k], 4 * mcse, n_eff)
        sq = (x - mean[k]) ** 2
        n_sq = ess(sq)
        assert n_sq > 100, (name, "variance", n_sq)
        mcse_v = math.sqrt(max(m4[k] - var[k] ** 2, 1e-300) / n_sq)
        assert abs(sq.mean() - var[k]) < 4.0 * mcse_v, "Var[%s] = %.5f, exact %.5f, 4 MCSE = %.5f" % (name, sq.mean(), var[k], 4 * mcse_v)
    V = q[:, 3:]
    for k in range(V.shape[1]):
        n_eff = ess(V[:, k])
        assert n_eff > 100, ("v[%d]" % k, n_eff)
        mcse = math.sqrt(P["v_var"][k] / n_eff)
        assert abs(V[:, k].mean() - P["v_mean"][k]) < 4.0 * mcse, "E[v_%d] = %.4f, exact %.4f, 4 MCSE = %.4f (ESS %.0f)" % (
            k, V[:, k].mean(), P["v_mean"][k], 4 * mcse, n_eff)


# ---------------------------------------------------------------------------------------------
# 7. train_sgp_hmc / predict_sgpmc end to end, the metric and the intervals
# ---------------------------------------------------------------------------------------------
def test_train_and_predict_end_to_end_over_the_double():
    rng = np.random.default_rng(2)
    X = np.sort(rng.uniform(-3.0, 3.0, 60))[:, None]
    Y = np.sin(2.0 * X[:, 0]) + 0.2 * rng.standard_normal(60)
    Z0 = np.linspace(-2.5, 2.5, 6)[:, None]
    Xs = np.linspace(-3.0, 3.0, 25)[:, None]
    model, trace, secs = ggp_amd.train_sgp_hmc((X, Y[:, None]), Z0, 1, 15, 15, engine=SgpmcOracleEngine(), seed=9, warmup_iters=30)
    assert len(trace) == 15 and secs > 0.0
    w = model.warmup
    assert w["iterations"] > 0 and w["loss_end"] < w["loss_start"]                  # the warm-up lowers -logp ...
    Zw = model.Z.clone()
    assert Zw.shape == (6, 1) and not torch.equal(Zw, T(Z0))                        # ... moving Z as well
    assert trace["V"].shape == (15, 6) and trace["lengthscales"].shape == (15, 1) and trace["variance"].shape == (15,)
    pred_mean, f_means, y_stds = ggp_amd.predict_sgpmc(model, trace, Xs)
    assert pred_mean.shape == (25,) and f_means.shape == (15, 25) and y_stds.shape == (15, 25)
    assert torch.equal(model.Z, Zw)                                                # Z is frozen while sampling and predicting
    assert np.allclose(pred_mean, f_means.mean(0)) and np.all(y_stds > 0.0)
    assert ggp_amd.predict_sgpmc(model, trace, Xs, n_draws=4)[1].shape == (4, 25)
    # the predictive of one draw, restated: mean = a^T v, var = k** - |a|^2 + noise variance
    row = trace[0]
    ls, sf2 = T(row["lengthscales"]), float(row["variance"])
    a = torch.linalg.solve_triangular(torch.linalg.cholesky(O.kuu(Zw, ls, sf2, 1e-5, 0)), O.kern(Zw, T(Xs), ls, sf2, 0), upper=False)
    assert np.allclose(f_means[0], (a.T @ T(row["V"])).numpy(), atol=1e-12)
    assert np.allclose(y_stds[0] ** 2, (sf2 - (a * a).sum(0)).numpy() + float(row["noise_variance"]), atol=1e-12)


def test_mixture_metric_and_intervals_on_a_two_component_example():
    # two components N(-1, 0.5^2) and N(2, 1^2), two test points y = 0 and y = 1, Y_std = 2
    loc = np.array([[-1.0, -1.0], [2.0, 2.0]])
    std = np.array([[0.5, 0.5], [1.0, 1.0]])
    y = np.array([0.0, 1.0])
    lp = lambda t, m, s: -0.5 * math.log(2 * math.pi * s * s) - 0.5 * ((t - m) / s) ** 2
    per_point = [0.5 * (lp(t, -1.0, 0.5) + lp(t, 2.0, 1.0)) - math.log(2.0) for t in y]
    want = -round(float(np.mean(per_point)), 3)
    assert ggp_amd.negative_log_predictive_mixture_density(y, loc, std, 2.0) == pytest.approx(want, abs=1e-12)
    assert ggp_amd.negative_log_predictive_mixture_density(torch.tensor(y)[:, None], loc, std, torch.tensor([2.0])) == pytest.approx(want, abs=1e-12)
    lo, hi = ggp_amd.get_posterior_predictive_uncertainty_intervals(loc, std)
    Phi = lambda t: 0.5 * (1.0 + math.erf(t / math.sqrt(2.0)))
    cdf = lambda t: 0.5 * (Phi((t + 1.0) / 0.5) + Phi((t - 2.0) / 1.0))
    assert lo.shape == hi.shape == (2,) and lo[0] == lo[1] and hi[0] == hi[1]
    assert cdf(lo[0]) == pytest.approx(0.025, abs=1e-12) and cdf(hi[0]) == pytest.approx(0.975, abs=1e-12)
    # the two components barely overlap: the 2.5 % point is the 5 % point of the left one, the 97.5 % point the 95 % point of the right one
    assert lo[0] == pytest.approx(-1.0 - 0.5 * 1.6448536269514722, abs=1e-3) and hi[0] == pytest.approx(2.0 + 1.6448536269514722, abs=1e-3)
    # one component: the Gaussian's own quantiles
    lo1, hi1 = ggp_amd.get_posterior_predictive_uncertainty_intervals(np.array([[0.3]]), np.array([[2.0]]))
    assert lo1[0] == pytest.approx(0.3 - 2.0 * 1.959963984540054, abs=1e-9) and hi1[0] == pytest.approx(0.3 + 2.0 * 1.959963984540054, abs=1e-9)
