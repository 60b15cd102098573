"""all_in_HMC on the GPU: the single-launch joint target (theta and Z) against an autograd yardstick built from the oracle, the
persistent joint sampler (sgp_small_nuts_joint) against host-driven hmc.NUTS over the same evaluations, and the model end to end
on Boston-shaped data."""
import math
import time

import numpy as np
import pytest
import torch

from conftest import dev, load_golden
from oracle import vfe_oracle as O


def _yardstick(G, q, kernel_id):
    """logp and its gradient over (theta, Z): oracle.vfe_pymc3_order + the theta priors / Jacobians + Z ~ Normal(0, 1)."""
    X = torch.as_tensor(np.asarray(G["X"]), dtype=torch.float64)
    y = torch.as_tensor(np.asarray(G["y"]), dtype=torch.float64).reshape(-1)
    M, d = np.asarray(G["Z"]).shape
    qt = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    ls, sf, sn = torch.exp(qt[:d]), torch.exp(qt[d]), torch.exp(qt[d + 1])
    Z = qt[d + 2:].reshape(M, d)
    F = O.vfe_pymc3_order(X, y, Z, ls, sf, sn, jitter=1e-6, kernel_id=kernel_id)
    c = math.log(2.0) - math.log(math.pi)
    lp = F + torch.sum(torch.log(ls) - ls) + (c - torch.log1p(sf * sf)) + (c - torch.log1p(sn * sn)) + torch.sum(qt[:d + 2])
    lp = lp - 0.5 * torch.sum(Z * Z) - 0.5 * math.log(2.0 * math.pi) * M * d
    lp.backward()
    return float(lp.detach()), qt.grad.numpy().copy()


def _start(G, rng):
    M, d = np.asarray(G["Z"]).shape
    return np.concatenate([np.log(np.asarray(G["ls"], dtype=np.float64).reshape(-1)) + 0.05 * rng.standard_normal(d),
                           [0.5 * math.log(float(G["sf2"])), 0.5 * math.log(float(G["s2"]))], np.asarray(G["Z"]).reshape(-1)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rbf_d1_tiny", "rbf_d3_small", "rbf_d18_mid", "m32_d2_small"])
def test_single_launch_joint_target_matches_the_yardstick(engine, name):
    import ggp_amd
    G = load_golden(name)
    kid = int(G["kernel_id"])
    kernel = {0: "rbf", 1: "matern32", 2: "matern52"}[kid]
    cb = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), kernel=kernel, jitter=1e-6, engine=engine)
    M = np.asarray(G["Z"]).shape[0]
    tgt = ggp_amd.JointHmcTarget(cb, M)
    assert cb._small_ok(M, want_gz=True)
    q = _start(G, np.random.default_rng(1))
    lp, g = tgt.logp_and_grad(q)
    lp_ref, g_ref = _yardstick(G, q, kid)
    print("%s: logp to %.1e relative" % (name, abs(lp - lp_ref) / abs(lp_ref)))
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    if kid == 0:
        assert np.allclose(g, g_ref, rtol=1e-7, atol=1e-7 * np.max(np.abs(g_ref)))
    else:  # autograd through the Matern profile is NaN at r = 0 (the diagonal of Kuu): central differences of the yardstick instead
        d = np.asarray(G["Z"]).shape[1]
        first_ls, log_sig_n, first_z, last_z = 0, d + 1, d + 2, len(q) - 1
        for i in (first_ls, log_sig_n, first_z, last_z):
            h = 1e-5
            qp, qm = q.copy(), q.copy()
            qp[i] += h
            qm[i] -= h
            fd = (_yardstick(G, qp, kid)[0] - _yardstick(G, qm, kid)[0]) / (2 * h)
            assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i]))


def _host_chain(tgt, q0, tune, draws, seed, depth):
    """hmc.NUTS with the wide sampler's dot-product order (FixedOrderNUTS), driven from the host over the single-launch target."""
    from ggp_amd.hmc import DiagMassAdapter, SplitMix
    from test_all_in_hmc import FixedOrderNUTS
    nuts = FixedOrderNUTS(tgt.logp_and_grad, tgt.ndim, max_treedepth=depth, rng=SplitMix(seed))
    q = q0.copy()
    lp, g = nuts._eval(q)
    nuts.mass = DiagMassAdapter(tgt.ndim, initial_mean=q)
    rows, sizes, steps, lps = [], [], [], []
    for it in range(tune + draws):
        q, lp, g, st = nuts.draw(q, lp, g, it < tune)
        if it >= tune:
            rows.append(q.copy())
            sizes.append(st["tree_size"])
            steps.append(st["step_size"])
            lps.append(lp)
    return np.array(rows), np.array(sizes, dtype=np.float64), np.array(steps), np.array(lps), nuts.n_leapfrog


@pytest.mark.gpu
@pytest.mark.parametrize("name,M,d,N", [("rbf_d3_small", None, None, None), ("rbf_d18_mid", None, None, None),
                                        ("synthetic", 128, 8, 700)])
def test_device_joint_nuts_matches_the_host_driven_sampler(engine, name, M, d, N):
    """sgp_small_nuts_joint against hmc.NUTS over the single-launch joint target, same splitmix stream: identical trees and
    evaluation counts; the first, untuned transitions to 1e-9 (M <= 64 and M = 128 instantiations; ndim 1 034 for the synthetic case)."""
    import ggp_amd
    if name == "synthetic":
        rng = np.random.default_rng(5)
        Xh = rng.standard_normal((N, d))
        yh = np.sin(Xh[:, 0]) + 0.5 * Xh[:, 1] + 0.1 * rng.standard_normal(N)
        G = {"X": Xh, "y": yh, "Z": Xh[:M].copy(), "ls": np.full(d, 2.0), "sf2": 1.0, "s2": 0.05}
    else:
        G = load_golden(name)
    X, y = dev(G["X"], engine), dev(np.asarray(G["y"]).reshape(-1), engine)
    M = np.asarray(G["Z"]).shape[0]
    cb = ggp_amd.CollapsedBound(X, y, jitter=1e-6, engine=engine)
    tgt = ggp_amd.JointHmcTarget(cb, M)
    assert tgt.device_sampler_ok()
    if name == "synthetic":
        assert tgt.ndim > 1024
    q0 = _start(G, np.random.default_rng(2))
    seed, depth = 4321, 6
    # (1) the first transitions, before the stiff posterior can amplify rounding: no tuning, so the step size is the initial one
    # on both sides and every number must agree tightly -- a stale or partial gradient entry, a position overwritten early or a
    # wrong reduction would show here at once
    r = engine.small_nuts_joint(X, y, M, q0, 0, 3, seed, jitter=1e-6, max_treedepth=depth)
    assert r["info"] == 0 and r["draws"] == 3
    rows, sizes, steps, lps, nleap = _host_chain(tgt, q0, 0, 3, seed, depth)
    assert r["evaluations"] == nleap and np.array_equal(r["stats"][:, 1].numpy(), sizes)
    assert np.array_equal(r["stats"][:, 0].numpy(), steps)
    assert np.allclose(r["samples"].numpy(), rows, rtol=1e-9, atol=1e-10)
    # the logp column is PyMC3's model logp at the draw (the Z prior's constants included), as the host target computes it
    assert np.allclose(r["stats"][:, 6].numpy(), lps, rtol=1e-10, atol=0)
    # (2) a tuned run: the same trees and evaluation counts; the numbers drift apart over the run (the device math library's exp /
    # log / sin / cos against libm in the momentum draws and the adaptation, amplified along 20 tuning trajectories), bounded here
    tune, draws = 20, 15
    r = engine.small_nuts_joint(X, y, M, q0, tune, draws, seed, jitter=1e-6, max_treedepth=depth)
    assert r["info"] == 0 and r["draws"] == tune + draws
    rows, sizes, steps, lps, nleap = _host_chain(tgt, q0, tune, draws, seed, depth)
    dstep = float(np.max(np.abs(r["stats"][:, 0].numpy() / steps - 1.0)))
    ddraw = float(np.max(np.abs(r["samples"].numpy() - rows)))
    print("\n%s: ndim %d; tuned run: step sizes to %.1e relative, draws to %.1e; sampler %.1f us / evaluation %.1f us per leaf" % (
        name, tgt.ndim, dstep, ddraw, 1e6 * r["sampler_seconds"] / r["evaluations"], 1e6 * r["eval_seconds"] / r["evaluations"]))
    assert r["evaluations"] == nleap
    assert np.array_equal(r["stats"][:, 1].numpy(), sizes)
    assert dstep < 1e-4
    assert np.allclose(r["samples"].numpy(), rows, rtol=1e-3, atol=1e-3)
    assert np.all(r["seconds"].numpy() > 0.0)


@pytest.mark.gpu
def test_all_in_hmc_on_boston_shaped_data(engine):
    """N 404, d 13, M 100 (the reference's Boston setting), 30 tune + 20 draws on the device: the mixture beats the training mean."""
    import ggp_amd
    rng = np.random.default_rng(11)
    N, d, M, T = 404, 13, 100, 102
    Xa = rng.standard_normal((N + T, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    ya = np.sin(Xa @ w * 2.0) + 0.3 * Xa[:, 0] + 0.1 * rng.standard_normal(N + T)
    ya = (ya - ya[:N].mean()) / ya[:N].std()
    X, y = dev(Xa[:N], engine), dev(ya[:N], engine)
    Xs = dev(Xa[N:], engine)
    m = ggp_amd.all_in_HMC(X, y, ggp_amd.GaussianLikelihood(), dev(Xa[:M], engine), engine=engine, seed=7)
    t0 = time.perf_counter()
    tr = m.sample(20, d, 30)
    wall = time.perf_counter() - t0
    assert getattr(tr, "device_resident", False)
    assert tr['Z'].shape == (20, M, d)
    preds = ggp_amd.full_mixture_posterior_predictive(m, Xs, tr)
    assert len(preds) > 0
    mu = torch.stack([p.mean.detach().to("cpu") for p in preds]).mean(0).numpy()
    rmse = float(np.sqrt(np.mean((mu - ya[N:]) ** 2)))
    base = float(np.sqrt(np.mean((ya[:N].mean() - ya[N:]) ** 2)))
    assert math.isfinite(rmse) and rmse < base
    print("boston-shaped joint NUTS: %d leapfrogs in %.2f s = %.1f leapfrogs/s; RMSE %.3f (training mean %.3f)" % (
        tr.n_leapfrog, wall, tr.n_leapfrog / wall, rmse, base))


@pytest.mark.gpu
def test_mixture_predict_with_a_z_per_sample(engine):
    """sgp_mixture_predict_zs: S = 11 (two chunks of at most eight), a distinct Z per sample: mean, variance and covariance
    against oracle.predict per sample, the PSD gate's statuses, and with every Z equal the bits of sgp_mixture_predict."""
    rng = np.random.default_rng(3)
    N, T, M, d, S = 300, 40, 20, 3, 11
    Xh = rng.standard_normal((N, d))
    yh = np.sin(Xh[:, 0]) + 0.2 * Xh[:, 1] + 0.1 * rng.standard_normal(N)
    Xsh = rng.standard_normal((T, d))
    Zs = rng.standard_normal((S, M, d))
    ls = [list(np.exp(rng.uniform(-0.3, 0.5, d))) for _ in range(S)]
    sf2 = [float(v) for v in np.exp(rng.uniform(-0.5, 0.5, S))]
    s2 = [float(v) for v in np.exp(rng.uniform(-4.0, -1.0, S))]
    X, y, Xs = dev(Xh, engine), dev(yh, engine), dev(Xsh, engine)
    r = engine.mixture_predict(X, y, Xs, dev(Zs, engine), ls, sf2, s2, jitter=1e-6, full_cov=True, gate_jitter=1e-5)
    assert np.all(r["info"].cpu().numpy() == 0) and np.all(r["gate"].cpu().numpy() == 0)
    for s in range(S):
        mu, cov = O.predict(torch.as_tensor(Xsh), torch.as_tensor(Xh), torch.as_tensor(yh), torch.as_tensor(Zs[s]),
                            torch.as_tensor(ls[s]), sf2[s], s2[s], jitter=1e-6, full_cov=True)
        assert np.allclose(r["mean"][s].cpu().numpy(), mu.numpy(), rtol=1e-9, atol=1e-9 * float(mu.abs().max()))
        assert np.allclose(r["cov"][s].cpu().numpy(), cov.numpy(), rtol=1e-9, atol=1e-9 * float(cov.abs().max()))
        assert np.allclose(r["var"][s].cpu().numpy(), np.diag(cov.numpy()), rtol=1e-9, atol=1e-9 * float(cov.abs().max()))
    # a sample whose predictive covariance fails the gate: a negative noise-free covariance shift (gate_jitter < 0)
    bad = engine.mixture_predict(X, y, Xs, dev(Zs, engine), ls, sf2, s2, jitter=1e-6, full_cov=True, gate_jitter=-10.0)
    assert np.all(bad["gate"].cpu().numpy() > 0)
    # every Z equal: the bits of the one-Z entry
    same = np.broadcast_to(Zs[0], (S, M, d)).copy()
    a = engine.mixture_predict(X, y, Xs, dev(same, engine), ls, sf2, s2, jitter=1e-6, full_cov=True, gate_jitter=1e-5)
    b = engine.mixture_predict(X, y, Xs, dev(Zs[0], engine), ls, sf2, s2, jitter=1e-6, full_cov=True, gate_jitter=1e-5)
    for k in ("mean", "var", "cov", "info", "gate"):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
