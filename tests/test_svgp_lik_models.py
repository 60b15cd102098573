"""CPU: ``StochasticVariationalGP`` with the likelihoods that have no noise parameter -- ``PoissonLikelihood`` and
``BernoulliLikelihood(link="logit")`` -- at the model level: the name reaches the engine, the labels are mapped, the bound and its
gradients equal autograd of a dense statement, and the predictive goes through the likelihood's ``__call__``."""
import math

import numpy as np
import pytest
import torch

import ggp_amd
from fake_engine import OracleEngine
from sgpmc_lik_double import LIK, lik_terms

DT = torch.float64


def dense_elbo(Xb, yb, Z, ls, sf2, m, LS, N_total, jitter, lik):
    """mean_b E_q log p(y_b | f_b) - KL / N of the whitened SVGP (rbf), differentiable; (bound, sum of the expectations, KL)."""
    M = Z.shape[0]
    r2 = lambda a, b: (((a / ls)[:, None, :] - (b / ls)[None, :, :]) ** 2).sum(-1)
    K = sf2 * torch.exp(-0.5 * r2(Z, Z)) + jitter * torch.eye(M, dtype=DT)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(K), sf2 * torch.exp(-0.5 * r2(Z, Xb)), upper=False)
    Ls = torch.tril(LS)
    T = Ls.T @ A
    mu, v = A.T @ m, sf2 - (A * A).sum(0) + (T * T).sum(0)
    ell = lik_terms(LIK[lik], yb, mu, v, 1.0)[0]
    kl = 0.5 * ((m * m).sum() + (Ls * Ls).sum() - M - 2.0 * torch.log(torch.diagonal(Ls)).sum())
    return ell.mean() - kl / N_total, ell.sum(), kl


class LikSvgpEngine(OracleEngine):
    """``OracleEngine`` whose SVGP bound also takes the two new likelihood names: autograd of ``dense_elbo`` (rbf)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def svgp_elbo(self, Xb, yb, Z, ls, sf2, s2, m, LS, N_total, jitter=1e-6, kernel="rbf", likelihood="gaussian", with_grads=False):
        self.seen.append((likelihood, float(s2), yb.clone()))
        if likelihood not in ("poisson", "bernoulli_logit"):
            return super().svgp_elbo(Xb, yb, Z, ls, sf2, s2, m, LS, N_total, jitter, kernel, likelihood, with_grads)
        assert kernel == "rbf"
        leaf = lambda t: t.detach().clone().requires_grad_(True)
        Zt, lst, sft, mt, LSt = leaf(Z), leaf(self._ls(ls, Z.shape[1])), torch.tensor(float(sf2), dtype=DT, requires_grad=True), leaf(m), leaf(LS)
        with torch.enable_grad():      # (the models call the engine from inside an autograd Function, where grad mode is off)
            F, es, kl = dense_elbo(Xb, yb, Zt, lst, sft, mt, LSt, N_total, jitter, likelihood)
        res = {"out": torch.stack([F, es, kl]).detach(), "info": torch.zeros(1, dtype=torch.int32)}
        if with_grads:
            gZ, gl, gs, gm, gL = torch.autograd.grad(F, (Zt, lst, sft, mt, LSt))
            res.update(g_m=gm, g_LS=torch.tril(gL), g_Z=gZ, g_ls=gl, g_sf2=gs.reshape(1), g_s2=torch.zeros(1, dtype=DT))
        return res


def problem(lik, N=90, M=7, d=2, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, d))
    f = np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, 1])
    y = rng.poisson(np.exp(f)).astype(np.float64) if lik == "poisson" else (f + 0.3 * rng.standard_normal(N) > 0).astype(np.float64)
    return torch.as_tensor(X), torch.as_tensor(y), torch.as_tensor(X[rng.choice(N, M, replace=False)].copy())


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("lik", ["poisson", "bernoulli_logit"])
def test_bound_gradients_and_predictive_through_the_model(lik, batched):
    X, y, Z0 = problem(lik)
    likelihood = ggp_amd.PoissonLikelihood() if lik == "poisson" else ggp_amd.BernoulliLikelihood(link="logit")
    eng = LikSvgpEngine()
    model = ggp_amd.StochasticVariationalGP(X, y, likelihood, Z0, engine=eng)
    model.batched = batched
    assert model._noise_free()
    with torch.no_grad():
        model.variational_mean.copy_(0.3 * torch.randn(7, dtype=DT, generator=torch.Generator().manual_seed(1)))
    xb, yb = X[:40], y[:40]
    loss = model.elbo_minibatch(xb, yb)
    loss.backward()
    name, s2, y_seen = eng.seen[-1]
    assert name == lik and s2 == 1.0
    y_want = yb if lik == "poisson" else torch.where(yb > 0, 1.0, -1.0).to(DT)      # {0, 1} labels -> {-1, +1}; counts untouched
    assert torch.equal(y_seen.reshape(-1), y_want)
    # the same bound densely, differentiated with respect to the model's own tensors
    Zt, mt, LSt = (t.detach().clone().requires_grad_(True) for t in (model.inducing_inputs, model.variational_mean,
                                                                     model.chol_variational_covar))
    ls = model.covar_module.base_kernel.lengthscale.detach().reshape(-1)
    sf2 = model.covar_module.outputscale.detach()
    F = dense_elbo(xb, y_want, Zt, ls, sf2, mt, LSt, model.num_data, model.jitter, lik)[0]
    gZ, gm, gL = torch.autograd.grad(F, (Zt, mt, LSt))
    assert abs(float(loss.detach()) - float(F.detach())) <= 1e-12 * (1.0 + abs(float(F.detach())))
    assert torch.allclose(model.inducing_inputs.grad, gZ, rtol=1e-9, atol=1e-12)
    assert torch.allclose(model.variational_mean.grad, gm, rtol=1e-9, atol=1e-12)
    assert torch.allclose(torch.tril(model.chol_variational_covar.grad), torch.tril(gL), rtol=1e-9, atol=1e-12)
    raw = [p for n, p in model.named_parameters() if "raw" in n and p.grad is not None]
    assert raw and all(bool(torch.isfinite(p.grad).all()) for p in raw) and any(float(p.grad.abs().max()) > 0 for p in raw)
    # the predictive through the likelihood: mean count exp(mu + v / 2), or the 20-point rule's class-1 probability
    pred = model.posterior_predictive(X[:9])
    mu, v = model.latent_predictive(X[:9])
    if lik == "poisson":
        assert torch.allclose(pred, torch.exp(mu + 0.5 * v)) and bool((pred > 0).all())
    else:
        gx, gw = np.polynomial.hermite.hermgauss(20)
        f = mu[:, None] + torch.sqrt(v)[:, None] * torch.as_tensor(gx * math.sqrt(2.0))
        assert torch.allclose(pred, torch.sigmoid(f) @ torch.as_tensor(gw / math.sqrt(math.pi)), rtol=1e-12)
        assert bool(((pred > 0) & (pred < 1)).all())


def test_training_loop_runs_with_a_noise_free_likelihood():
    X, y, Z0 = problem("poisson")
    model = ggp_amd.StochasticVariationalGP(X, y, ggp_amd.PoissonLikelihood(), Z0, engine=LikSvgpEngine())
    batches = [(X[i:i + 30], y[i:i + 30]) for i in (0, 30, 60)]
    losses = model.train_model(torch.optim.Adam(model.parameters(), lr=0.05), batches, num_epochs=3)
    losses = losses[-1] if isinstance(losses, tuple) else losses
    # one entry per minibatch: the last epoch's three against the first epoch's
    assert len(losses) == 9 and all(math.isfinite(float(t)) for t in losses) and sum(losses[-3:]) < sum(losses[:3])
