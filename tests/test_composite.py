"""Sum-of-products covariances: oracle self-consistency, golden fixtures, the host-side kernel
description / NUTS target, the dataset readers (CPU); HIP parity through the C ABI (``-m gpu``)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, dev
from oracle import composite_oracle as CO
from oracle import vfe_oracle as O

COMP_DIR = os.path.join(GOLDEN_DIR, "composite")


def comp_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(COMP_DIR, "*.npz")))


def load_comp(name):
    z = np.load(os.path.join(COMP_DIR, name + ".npz"))
    return {k: z[k] for k in z.files}


def _problem(N=120, M=9, d=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, d, dtype=torch.float64, generator=g) * 8.0
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    return X, y, X[:M].clone()


# ------------------------------------------------------------------------------------------------ CPU
def test_single_factor_composites_equal_the_plain_kernels():
    X, y, Z = _problem(d=2)
    for ty, kid in ((CO.EXPQUAD, O.KERNEL_RBF), (CO.MATERN32, O.KERNEL_MATERN32), (CO.MATERN52, O.KERNEL_MATERN52)):
        blk = CO.make_block([(1.7, [(ty, 0.9)])])
        Fc = float(CO.vfe_composite(X, y, Z, blk, 0.05, 1e-6))
        Fp = float(O.vfe_pymc3_order(X, y, Z, [0.9, 0.9], math.sqrt(1.7), math.sqrt(0.05), 1e-6, kid))
        assert abs(Fc - Fp) < 1e-9 * max(1.0, abs(Fp))


def test_oracle_gradients_match_finite_differences():
    X, y, Z = _problem()
    blk = CO.co2_block(n_per=0.8, l_psmooth=1.3, l_pdecay=3.0, n_med=0.5, l_med=1.1, alpha=0.7, n_trend=1.5, l_trend=2.0,
                       n_noise=0.3, l_noise=0.4)
    F, g = CO.vfe_composite_and_grads(X, y, Z, blk, 0.04)
    for i in CO.grad_slots(blk):
        e = np.zeros(CO.COMP_LEN)
        e[i] = 1e-6 * max(1.0, abs(blk[i]))
        fd = (float(CO.vfe_composite(X, y, Z, blk + e, 0.04)) - float(CO.vfe_composite(X, y, Z, blk - e, 0.04))) / (2 * e[i])
        assert abs(fd - float(g["block"][i])) < 1e-5 * max(1.0, abs(fd)), (i, fd, float(g["block"][i]))


@pytest.mark.parametrize("name", comp_names())
def test_oracle_reproduces_composite_golden(name):
    G = load_comp(name)
    F, g = CO.vfe_composite_and_grads(G["X"], G["y"], G["Z"], G["block"], float(G["s2"]), float(G["jitter"]))
    assert abs(F - float(G["F"])) < 1e-9 * max(1.0, abs(float(G["F"])))
    assert np.allclose(g["block"].numpy(), G["g_block"], rtol=1e-7, atol=1e-9)
    mu, cov = CO.predict_composite(G["Xs"], G["X"], G["y"], G["Z"], G["block"], float(G["s2"]), float(G["jitter"]))
    assert np.allclose(mu.numpy(), G["pred_mean"], atol=1e-9) and np.allclose(cov.numpy(), G["pred_cov"], atol=1e-9)


def test_composite_kernel_block_layout_and_round_trip():
    import ggp_amd
    k = ggp_amd.co2_kernel(n_per=0.8, l_psmooth=1.3, l_pdecay=3.0, n_med=0.5, l_med=1.1, alpha=0.7, n_trend=1.5, l_trend=2.0,
                           n_noise=0.3, l_noise=0.4)
    ref = CO.co2_block(n_per=0.8, l_psmooth=1.3, l_pdecay=3.0, n_med=0.5, l_med=1.1, alpha=0.7, n_trend=1.5, l_trend=2.0,
                       n_noise=0.3, l_noise=0.4)
    assert np.allclose(k.block(), ref)
    names = [n for n, _, _ in k.free_parameters()]
    assert names == ["amp_0", "ls_0_0", "ls_0_1", "amp_1", "ls_1_0", "aux_1_0", "amp_2", "ls_2_0", "amp_3", "ls_3_0"]  # period pinned
    assert set(names) == set(ggp_amd.CO2_LOG_PRIOR_SD)
    assert np.allclose(k.with_values(k.values()).block(), ref)
    with pytest.raises(ValueError):
        ggp_amd.CompositeKernel([(1.0, [ggp_amd.Factor("rbf", 1.0)] * 3)])


class _OracleCompositeBound:
    """Duck-typed stand-in for CollapsedBound(kernel='composite') on the CPU (test double, lives under tests/)."""
    kernel = "composite"

    def __init__(self, X, y):
        self.X, self.y = X, y

    def _prep_Z(self, Z):
        return torch.as_tensor(Z, dtype=torch.float64)

    def value_and_grad(self, Z, block, sf2, s2, want_gz=False, raise_on_fail=True):
        F, g = CO.vfe_composite_and_grads(self.X, self.y, Z, np.asarray(block), s2, 1e-6)
        return F, {"ls": g["block"], "sf2": 0.0, "s2": g["s2"], "Z": None, "info": 0}


def test_composite_hmc_target_priors_and_chain_rule():
    import ggp_amd
    X, y, Z = _problem(N=80, M=7)
    kern = ggp_amd.co2_kernel()
    tgt = ggp_amd.CompositeHmcTarget(_OracleCompositeBound(X, y), Z, kern, ggp_amd.CO2_LOG_PRIOR_SD)
    g = torch.Generator().manual_seed(1)
    th = (0.3 * torch.randn(tgt.ndim, dtype=torch.float64, generator=g)).tolist()
    lp, grad = tgt.logp_and_grad(th)
    # value: bound + Normal log-densities of the log-parameters + HalfNormal(1) on sigma with its log-Jacobian
    vals = [math.exp(v) for v in th[:-1]]
    sigma = math.exp(th[-1])
    F = float(CO.vfe_composite(X, y, Z, np.asarray(kern.with_values(vals).block()), sigma ** 2, 1e-6))
    prior = sum(-0.5 * (t / sd) ** 2 - math.log(sd) - 0.5 * math.log(2 * math.pi) for t, sd in zip(th[:-1], tgt.sd))
    prior += 0.5 * math.log(2 / math.pi) - 0.5 * sigma ** 2 + th[-1]
    assert abs(lp - (F + prior)) < 1e-9 * max(1.0, abs(lp))
    for i in range(tgt.ndim):  # gradient by central differences of logp
        e = [0.0] * tgt.ndim
        e[i] = 1e-6
        fd = (tgt.logp([a + b for a, b in zip(th, e)]) - tgt.logp([a - b for a, b in zip(th, e)])) / 2e-6
        assert abs(fd - grad[i]) < 1e-5 * max(1.0, abs(fd)), (i, fd, grad[i])
    assert tgt.logp([1000.0] * tgt.ndim) == -math.inf
    c = tgt.constrain(tgt.start())
    assert c["sig_n"] == 1.0 and len(c["ls"]) == tgt.ndim - 1


def test_dataset_readers(tmp_path):
    import ggp_amd
    from scipy.io import savemat
    rng = np.random.RandomState(0)
    yrs = 1958.0 + np.arange(700) / 12.0
    co2 = 315.0 + 1.5 * (yrs - 1958.0) + 3.0 * np.sin(2 * np.pi * yrs)
    co2[[5, 77]] = -99.99
    p = tmp_path / "mauna.txt"
    p.write_text("".join("%.4f   %.2f\n" % (a, b) for a, b in zip(yrs, co2)))
    y_tr, t_tr, y_te, t_te, std = ggp_amd.datasets.load_co2_dataset(str(p), 2010)
    assert t_tr.shape == (634, 1) and y_te.shape == (60,) and t_tr[0, 0] == 0.0 and y_tr[0] == 0.0
    keep = np.array([float("%.2f" % v) for v in np.delete(co2, [5, 77])])
    assert abs(std - np.std(keep)) < 1e-12 and abs(y_tr[10] - (keep[10] - keep[0]) / std) < 1e-12
    data = rng.randn(200, 19)
    savemat(str(tmp_path / "elevators.mat"), {"data": data})
    X, Y = ggp_amd.datasets.read_elevators_mat(str(tmp_path / "elevators.mat"))
    assert X.shape == (200, 18) and Y.shape == (200, 1) and np.allclose(Y[:, 0], data[:, -1])
    Xtr, ytr, Xte, yte = ggp_amd.datasets.split_dataset(X, Y, split=3)
    assert Xtr.shape == (180, 18) and yte.shape == (20,)
    ind = np.arange(200)
    np.random.RandomState(3).shuffle(ind)
    assert np.allclose(Xtr[0], ((X - X.mean(0)) / (1e-6 + X.std(0)))[ind[0]])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", comp_names())
def test_composite_bound_grads_predict_golden(engine, name):
    import ggp_amd
    G = load_comp(name)
    blk = G["block"].tolist()
    cb = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), kernel="composite", jitter=float(G["jitter"]), engine=engine)
    Z = dev(G["Z"], engine)
    F, _ = cb.value(Z, blk, 1.0, float(G["s2"]))
    tolF = 1e-8 * max(1.0, abs(float(G["F"])))  # north_star tolerance; the CO2 fixture's cond(Kuu) is ~1e5
    assert abs(F - float(G["F"])) < tolF, (F, float(G["F"]))
    F2, g = cb.value_and_grad(Z, blk, 1.0, float(G["s2"]), want_gz=True)  # dF/dZ: the materialised multi-launch path
    assert abs(F2 - F) < tolF and g["sf2"] == 0.0
    sl = CO.grad_slots(G["block"])
    gb = g["ls"].numpy()
    assert np.abs(gb[sl] - G["g_block"][sl]).max() < 1e-6 * max(1.0, np.abs(G["g_block"][sl]).max())
    assert np.all(gb[[i for i in range(CO.COMP_LEN) if i not in sl and i not in (1, 9, 17, 25)]] == 0.0)
    assert abs(g["s2"] - float(G["g_s2"])) < 1e-6 * max(1.0, abs(float(G["g_s2"])))
    assert (g["Z"].cpu().numpy() - G["g_Z"]).__abs__().max() < 1e-5 * max(1.0, np.abs(G["g_Z"]).max())
    mean, var, cov = cb.predict(dev(G["Xs"], engine), Z, blk, 1.0, float(G["s2"]), full_cov=True)
    assert np.abs(mean.cpu().numpy() - G["pred_mean"]).max() < 1e-7
    assert np.abs(cov.cpu().numpy() - G["pred_cov"]).max() < 1e-7
    assert np.abs(var.cpu().numpy() - np.diag(G["pred_cov"])).max() < 1e-7


@pytest.mark.gpu
def test_composite_rejects_bad_blocks_and_large_d(engine):
    import ggp_amd
    X, y, Z = _problem(d=2)
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), kernel="composite", jitter=1e-6, engine=engine)
    bad = CO.make_block([(1.0, [(CO.EXPQUAD, 1.0)])])
    bad[1] = -1.0  # negative amplitude
    with pytest.raises(ggp_amd.SgpStatusError):
        cb.value(Z.to(engine.device), bad.tolist(), 1.0, 0.1)
    with pytest.raises(ValueError):
        cb.value(Z.to(engine.device), [1.0, 1.0], 1.0, 0.1)  # not a parameter block
    X9 = torch.randn(50, 9, dtype=torch.float64).to(engine.device)
    cb9 = ggp_amd.CollapsedBound(X9, y[:50].to(engine.device), kernel="composite", jitter=1e-6, engine=engine)
    with pytest.raises(ggp_amd.SgpStatusError):
        cb9.value(X9[:5].clone(), CO.make_block([(1.0, [(CO.EXPQUAD, 1.0)])]).tolist(), 1.0, 0.1)


@pytest.mark.gpu
def test_composite_chunked_rows_match_oracle(engine):
    """More rows than one materialised chunk (65536) and more than one gradient block per chunk."""
    import ggp_amd
    g = torch.Generator().manual_seed(5)
    N, M = 70_000, 40
    X = torch.rand(N, 1, dtype=torch.float64, generator=g) * 30.0
    y = torch.sin(X[:, 0]) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    blk = CO.make_block([(1.1, [(CO.PERIODIC, 1.2, 6.3), (CO.EXPQUAD, 20.0)]), (0.3, [(CO.MATERN32, 0.8)])])
    F0, g0 = CO.vfe_composite_and_grads(X, y, Z, blk, 0.02, 1e-6)
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), kernel="composite", jitter=1e-6, engine=engine)
    F1, g1 = cb.value_and_grad(Z.to(engine.device), blk.tolist(), 1.0, 0.02, want_gz=True)
    assert abs(F1 - F0) < 1e-8 * abs(F0)
    sl = CO.grad_slots(blk)
    assert (g1["ls"][sl] - g0["block"][sl]).abs().max() < 1e-6 * g0["block"][sl].abs().max()
    assert (g1["Z"].cpu() - g0["Z"]).abs().max() < 1e-5 * g0["Z"].abs().max()


@pytest.mark.gpu
def test_co2_nuts_on_device(engine):
    """The reference's CO2 NUTS stage (co2_bayesian_sgpr_hmc.py:99-158) on a synthetic Keeling-like series."""
    import ggp_amd
    g = torch.Generator().manual_seed(11)
    t = torch.linspace(0.0, 20.0, 240, dtype=torch.float64)[:, None]
    y = 0.15 * t[:, 0] + 0.3 * torch.sin(2 * math.pi * t[:, 0]) + 0.05 * torch.randn(240, dtype=torch.float64, generator=g)
    y = (y - y[0]) / y.std()
    Z = t[::12].clone()
    cb = ggp_amd.CollapsedBound(t.to(engine.device), y.to(engine.device), kernel="composite", jitter=1e-6, engine=engine)
    tgt = ggp_amd.CompositeHmcTarget(cb, Z.to(engine.device), ggp_amd.co2_kernel(), ggp_amd.CO2_LOG_PRIOR_SD)
    lp, grad = tgt.logp_and_grad(tgt.start())
    F, gg = CO.vfe_composite_and_grads(t, y, Z, np.asarray(ggp_amd.co2_kernel().block()), 1.0, 1e-6)
    prior = sum(-math.log(sd) - 0.5 * math.log(2 * math.pi) for sd in tgt.sd) + 0.5 * math.log(2 / math.pi) - 0.5
    assert abs(lp - (F + prior)) < 1e-8 * max(1.0, abs(lp))
    trace = ggp_amd.sample_nuts(tgt, n_samples=12, tune=30, seed=3, start=tgt.start())
    assert len(trace) == 12 and np.all(np.isfinite(trace.get_sampler_stats("logp")))
    assert np.all(trace["ls"] > 0) and trace["ls"].shape == (12, tgt.ndim - 1)
    assert trace.get_sampler_stats("logp").mean() > lp  # the sampler moved off the (poor) test point


# ---- the single launch (sgp_small_eval_composite) and the device-resident sampler over the composite target ---------
@pytest.mark.gpu
@pytest.mark.parametrize("name", comp_names())
def test_composite_single_launch_golden_and_multi_launch(engine, name):
    """M <= 128, no dF/dZ: ONE launch evaluates the composite bound; against the fixture and against the materialised path."""
    import ggp_amd
    G = load_comp(name)
    blk = G["block"].tolist()
    X, y, Z = dev(G["X"], engine), dev(G["y"], engine), dev(G["Z"], engine)
    if not engine.small_supported(X.shape[0], Z.shape[0], X.shape[1], "composite"):
        pytest.skip("fixture outside the single-launch size class")
    cb = ggp_amd.CollapsedBound(X, y, kernel="composite", jitter=float(G["jitter"]), engine=engine)
    assert cb._small_ok(Z.shape[0]) and not cb._small_ok(Z.shape[0], want_gz=True)
    F, g = cb.value_and_grad(Z, blk, 1.0, float(G["s2"]))
    tolF = 1e-8 * max(1.0, abs(float(G["F"])))
    assert abs(F - float(G["F"])) < tolF, (F, float(G["F"]))
    sl = CO.grad_slots(G["block"])
    gb = g["ls"].numpy()
    assert np.abs(gb[sl] - G["g_block"][sl]).max() < 1e-6 * max(1.0, np.abs(G["g_block"][sl]).max())
    assert np.all(gb[[i for i in range(CO.COMP_LEN) if i not in sl and i not in (1, 9, 17, 25)]] == 0.0)
    assert abs(g["s2"] - float(G["g_s2"])) < 1e-6 * max(1.0, abs(float(G["g_s2"])))
    Fv, parts = cb.value(Z, blk, 1.0, float(G["s2"]))
    assert Fv == F and abs(parts["logmarg"] - parts["trace_term"] - F) < 1e-9 * max(1.0, abs(F))
    cb.fused = False
    F2, g2 = cb.value_and_grad(Z, blk, 1.0, float(G["s2"]))
    assert abs(F2 - F) < tolF
    assert np.abs(gb[sl] - g2["ls"].numpy()[sl]).max() < 1e-6 * max(1.0, np.abs(gb[sl]).max())
    assert abs(g["s2"] - g2["s2"]) < 1e-6 * max(1.0, abs(g2["s2"]))


@pytest.mark.gpu
def test_composite_single_launch_rejects_bad_arguments(engine):
    import ggp_amd
    X, y, Z = _problem(d=2)
    X, y, Z = X.to(engine.device), y.to(engine.device), Z.to(engine.device)
    good = CO.make_block([(1.0, [(CO.EXPQUAD, 1.0)])]).tolist()
    th = torch.tensor(good + [0.1], dtype=torch.float64).to(engine.device)
    out, _, info = engine.small_eval(X, y, Z, th, 1e-6, "composite", composite={"structure": good})
    assert int(info.item()) == 0 and math.isfinite(float(out[0]))
    with pytest.raises(ValueError):
        engine.small_eval(X, y, Z, th, 1e-6, "composite")  # no structure
    with pytest.raises(ValueError):
        engine.small_eval(X, y, Z, th, 1e-6, "composite", want_gz=True, composite={"structure": good})
    bad = list(good)
    bad[3] = 9.0  # unknown factor type
    with pytest.raises(ggp_amd.SgpStatusError):
        engine.small_eval(X, y, Z, th, 1e-6, "composite", composite={"structure": bad})
    # free-parameter table: slot 2 is a structural slot (the factor count), not an amplitude
    thh = torch.zeros(2, dtype=torch.float64).to(engine.device)
    with pytest.raises(ggp_amd.SgpStatusError):
        engine.small_eval(X, y, Z, thh, 1e-6, "composite", mode=1, composite={"structure": good, "free": [(2, 0, 1.0)]})
    # a non-positive amplitude in theta: density zero (info 0, value -inf), like any theta outside the domain
    thb = th.clone()
    thb[1] = -1.0
    out, _, info = engine.small_eval(X, y, Z, thb, 1e-6, "composite", composite={"structure": good})
    assert float(out[0]) == -math.inf and int(info.item()) == 0


@pytest.mark.gpu
def test_composite_hmc_target_single_launch_equals_host_chain_rule(engine):
    """CompositeHmcTarget: transforms, priors and chain rule on the device (mode SGP_SMALL_HMC) against the host-side
    chain rule over the materialised path, and against the oracle at the test point."""
    import ggp_amd
    g = torch.Generator().manual_seed(11)
    t = torch.linspace(0.0, 20.0, 240, dtype=torch.float64)[:, None]
    y = 0.15 * t[:, 0] + 0.3 * torch.sin(2 * math.pi * t[:, 0]) + 0.05 * torch.randn(240, dtype=torch.float64, generator=g)
    y = (y - y[0]) / y.std()
    Z = t[::12].clone()
    cb = ggp_amd.CollapsedBound(t.to(engine.device), y.to(engine.device), kernel="composite", jitter=1e-6, engine=engine)
    tgt = ggp_amd.CompositeHmcTarget(cb, Z.to(engine.device), ggp_amd.co2_kernel(), ggp_amd.CO2_LOG_PRIOR_SD)
    assert tgt.device_sampler_ok()
    gen = torch.Generator().manual_seed(2)
    for k in range(3):
        th = (0.4 * torch.randn(tgt.ndim, dtype=torch.float64, generator=gen)).tolist()
        cb.fused = True
        lp1, g1 = tgt.logp_and_grad(th)
        cb.fused = False
        lp2, g2 = tgt.logp_and_grad(th)
        assert abs(lp1 - lp2) < 1e-8 * max(1.0, abs(lp2)), (lp1, lp2)
        assert np.max(np.abs(np.array(g1) - np.array(g2))) < 1e-6 * max(1.0, np.max(np.abs(g2))), (g1, g2)
    cb.fused = True
    assert tgt.logp([200.0] * tgt.ndim) == -math.inf


@pytest.mark.gpu
def test_composite_device_resident_nuts_matches_the_host_driven_sampler(engine):
    """sgp_small_nuts_composite against hmc.NUTS driven from the host with the same splitmix stream over the same
    single-launch target: identical trees, draws equal to rounding."""
    import ggp_amd
    from ggp_amd.hmc import NUTS, DiagMassAdapter, SplitMix
    g = torch.Generator().manual_seed(11)
    t = torch.linspace(0.0, 20.0, 240, dtype=torch.float64)[:, None]
    y = 0.15 * t[:, 0] + 0.3 * torch.sin(2 * math.pi * t[:, 0]) + 0.05 * torch.randn(240, dtype=torch.float64, generator=g)
    y = (y - y[0]) / y.std()
    X, yd, Z = t.to(engine.device), y.to(engine.device), t[::12].clone().to(engine.device)
    cb = ggp_amd.CollapsedBound(X, yd, kernel="composite", jitter=1e-6, engine=engine)
    tgt = ggp_amd.CompositeHmcTarget(cb, Z, ggp_amd.co2_kernel(), ggp_amd.CO2_LOG_PRIOR_SD)
    q0 = np.array(tgt.start()) + 0.05
    tune, draws, seed = 15, 10, 77
    r = engine.small_nuts(X, yd, Z, q0, tune, draws, seed, jitter=1e-6, kernel="composite", max_treedepth=6,
                          composite=tgt.device_description())
    assert r["info"] == 0 and r["draws"] == tune + draws
    nuts = NUTS(tgt.logp_and_grad, tgt.ndim, max_treedepth=6, rng=SplitMix(seed))
    q = q0.copy()
    lp, gr = nuts._eval(q)
    nuts.mass = DiagMassAdapter(tgt.ndim, initial_mean=q)
    rows, sizes = [], []
    for it in range(tune + draws):
        q, lp, gr, st = nuts.draw(q, lp, gr, it < tune)
        if it >= tune:
            rows.append(q.copy())
            sizes.append(st["tree_size"])
    assert r["evaluations"] == nuts.n_leapfrog
    assert np.array_equal(r["stats"][:, 1].numpy(), np.array(sizes, dtype=np.float64))
    assert np.allclose(r["samples"].numpy(), np.array(rows), rtol=1e-6, atol=1e-8)
    # and through the public wrapper: the trace surface of the host sampler
    tr = ggp_amd.sample_nuts_device(tgt, 20, 30, seed=5, start=tgt.start(), max_treedepth=6)
    assert len(tr) == 20 and tr["ls"].shape == (20, tgt.ndim - 1) and np.all(tr["ls"] > 0)
    assert np.all(np.isfinite(tr.get_sampler_stats("logp")))


@pytest.mark.gpu
def test_composite_single_launch_two_tile_size_class(engine):
    """64 < M <= 128 (two 64-wide tiles, two Kuu-adjoint workgroups): the launch against the oracle, the NUTS target against
    the host chain rule over the materialised path, and a short device-resident run (this instantiation once faulted)."""
    import ggp_amd
    g = torch.Generator().manual_seed(4)
    N, M = 634, 100
    t = torch.linspace(0.0, 30.0, N, dtype=torch.float64)[:, None]
    y = 0.15 * t[:, 0] + 0.3 * torch.sin(2 * math.pi * t[:, 0]) + 0.05 * torch.randn(N, dtype=torch.float64, generator=g)
    y = (y - y[0]) / y.std()
    Z = t[torch.linspace(0, N - 1, M).round().long()].clone()
    X, yd, Zd = t.to(engine.device), y.to(engine.device), Z.to(engine.device)
    kern = ggp_amd.co2_kernel(0.5, 1.0, 5.0, 1.0, 3.0, 1.0, 0.5, 2.0, 0.1, 0.5)
    blk = np.asarray(kern.block())
    cb = ggp_amd.CollapsedBound(X, yd, kernel="composite", jitter=1e-6, engine=engine)
    assert cb._small_ok(M)
    F0, g0 = CO.vfe_composite_and_grads(t, y, Z, blk, 0.05, 1e-6)
    F1, g1 = cb.value_and_grad(Zd, blk.tolist(), 1.0, 0.05)
    assert abs(F1 - float(F0)) < 1e-8 * max(1.0, abs(float(F0)))
    sl = CO.grad_slots(blk)
    assert (g1["ls"][sl] - g0["block"][sl]).abs().max() < 1e-6 * max(1.0, float(g0["block"][sl].abs().max()))
    assert abs(g1["s2"] - float(g0["s2"])) < 1e-6 * max(1.0, abs(float(g0["s2"])))
    tgt = ggp_amd.CompositeHmcTarget(cb, Zd, ggp_amd.co2_kernel(), ggp_amd.CO2_LOG_PRIOR_SD)
    th = [0.1] * tgt.ndim
    lp1, gr1 = tgt.logp_and_grad(th)
    cb.fused = False
    lp2, gr2 = tgt.logp_and_grad(th)
    cb.fused = True
    assert abs(lp1 - lp2) < 1e-8 * max(1.0, abs(lp2))
    assert np.max(np.abs(np.array(gr1) - np.array(gr2))) < 1e-6 * max(1.0, np.max(np.abs(gr2)))
    r = engine.small_nuts(X, yd, Zd, np.array(th), 8, 8, 5, jitter=1e-6, kernel="composite", max_treedepth=4,
                          composite=tgt.device_description())
    assert r["info"] == 0 and r["draws"] == 16 and np.all(np.isfinite(r["samples"].numpy()))


# ---- the reference's CO2 model class with the alternating schedule --------------------------------------------------
def _keeling(n=240, seed=11):
    g = torch.Generator().manual_seed(seed)
    t = torch.linspace(0.0, 20.0, n, dtype=torch.float64)[:, None]
    y = 0.15 * t[:, 0] + 0.3 * torch.sin(2 * math.pi * t[:, 0]) + 0.05 * torch.randn(n, dtype=torch.float64, generator=g)
    return t, (y - y[0]) / y.std()


@pytest.mark.gpu
def test_composite_model_class_gradients_match_finite_differences(engine):
    """-F/N of ``CompositeBayesianSparseGPR_HMC`` (experiments/co2_bayesian_sgpr_hmc.py:58-98 upstream): autograd through the
    raw softplus parameters, the noise and Z against central differences of the same loss."""
    import ggp_amd
    t, y = _keeling()
    model = ggp_amd.CompositeBayesianSparseGPR_HMC(t.to(engine.device), y.to(engine.device), ggp_amd.co2_kernel(0.5, 1.0, 5.0, 1.0, 3.0, 1.0, 0.5, 2.0, 0.1, 0.5),
                                                   t[::12].clone(), ggp_amd.CO2_LOG_PRIOR_SD, engine=engine, noise=0.05)
    loss = model.neg_bound_per_datum()
    loss.backward()
    g_raw, g_noise, g_Z = model.raw_values.grad.clone(), float(model.raw_noise.grad), model.inducing_points.grad.clone().cpu()

    def at(param, idx, h):
        with torch.no_grad():
            old = param.view(-1)[idx].clone()
            param.view(-1)[idx] = old + h
            v = float(model.neg_bound_per_datum())
            param.view(-1)[idx] = old
        return v

    for k in range(model.raw_values.numel()):
        fd = (at(model.raw_values, k, 1e-5) - at(model.raw_values, k, -1e-5)) / 2e-5
        assert abs(fd - float(g_raw[k])) < 2e-5 * max(1.0, abs(fd)), (k, fd, float(g_raw[k]))
    fd = (at(model.raw_noise, 0, 1e-5) - at(model.raw_noise, 0, -1e-5)) / 2e-5
    assert abs(fd - g_noise) < 2e-5 * max(1.0, abs(fd))
    for k in (0, 7, 19):
        fd = (at(model.inducing_points, k, 1e-5) - at(model.inducing_points, k, -1e-5)) / 2e-5
        assert abs(fd - float(g_Z.view(-1)[k])) < 2e-5 * max(1.0, abs(fd)), (k, fd, float(g_Z.view(-1)[k]))


@pytest.mark.gpu
def test_composite_model_class_alternating_schedule_on_device(engine):
    """Warm start (Adam on everything), then NUTS phases at the scheduled iterations with Adam on Z alone against the bound
    averaged over the trace (experiments/co2_bayesian_sgpr_hmc.py:186-253 upstream), the HMC-only run (:257-277) and the
    mixture predictive."""
    import ggp_amd
    t, y = _keeling()
    model = ggp_amd.CompositeBayesianSparseGPR_HMC(t.to(engine.device), y.to(engine.device), ggp_amd.co2_kernel(), t[::12].clone(),
                                                   ggp_amd.CO2_LOG_PRIOR_SD, engine=engine, seed=5)
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    raw0 = model.raw_values.detach().clone()
    losses, trace, steps, perf = model.train_model(opt, max_steps=46, hmc_scheduler=(30, 36, 42), num_tune_long=30, num_samples_long=8,
                                                   num_tune_short=10, num_samples_short=4)
    assert len(losses) == 30 + 15 and all(math.isfinite(v) for v in losses)  # iteration 30 samples first, then 15 averaged steps
    assert losses[29] < losses[0]                                            # the warm start optimises
    assert not torch.equal(model.raw_values.detach(), raw0)                 # ... and moved the kernel parameters
    assert len(trace) == 8 and len(steps) == 3 and len(perf) == 3 and all(s > 0 for s in steps)
    assert not model.raw_values.requires_grad and model.inducing_points.requires_grad
    assert trace["ls"].shape == (8, len(model.params)) and np.all(trace["ls"] > 0)
    Z_after = model.inducing_points.detach().cpu().clone()
    assert float((Z_after - t[::12]).abs().max()) > 0.0                      # Z kept moving in the frozen phase
    tr2, st2, pf2 = model.train_fixed_model(num_tune=20, num_samples=6)
    assert len(tr2) == 6 and st2[0] > 0 and pf2[0] > 0
    tt = torch.linspace(20.0, 22.0, 25, dtype=torch.float64)[:, None].to(engine.device)
    preds = model.mixture_posterior_predictive(tt, tr2)
    assert len(preds) == 6 and preds[0][0].shape == (25,) and bool(torch.all(preds[0][1] > 0))
    mean, var = model.posterior_predictive(tt)
    assert torch.equal(mean, preds[-1][0]) and bool(torch.isfinite(mean).all())


def test_composite_model_class_parameter_transforms():
    from ggp_amd.composite import _inv_softplus
    for v in (1e-6, 1e-3, 0.3, 2.0, 40.0):
        assert abs(math.log1p(math.exp(_inv_softplus(v))) - v) < 1e-12 * max(1.0, v) or v > 30.0


# ---- factored pass 2: the whitened order on ill-conditioned K_uu with M > 128 (the reference's CO2 run uses M = 480) -----
@pytest.mark.gpu
def test_factored_pass2_on_ill_conditioned_composite(engine):
    """cond(K_uu) ~ 2e10: with Phibar formed explicitly the gradient of the bound is off by 1e-2 .. 1e-1 (its cond-sized
    entries cancel in Phibar K_uf); applied factor by factor (sgp_suffstats_bwd_factored) it matches the oracle's autograd
    through the PyMC3 op order.  Values agree in both modes."""
    import ggp_amd
    sys_path_exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "experiments")
    import sys
    sys.path.insert(0, sys_path_exp)
    from co2_composite_hmc import synthetic_keeling
    y_tr, t_tr, _, _, _ = synthetic_keeling(seed=47)
    X, y = torch.as_tensor(t_tr, dtype=torch.float64), torch.as_tensor(y_tr, dtype=torch.float64)
    M = 200
    Z = X[torch.linspace(0, X.shape[0] - 1, M).round().long()].clone()
    blk = np.asarray(ggp_amd.co2_kernel(0.0745, 0.873, 6.45, 9.96, 136.0, 1.008, 0.0186, 6.83, 0.00065, 3.06).block())
    s2 = 0.0123 ** 2
    F0, g0 = CO.vfe_composite_and_grads(X, y, Z, blk, s2, 1e-6)
    sl = CO.grad_slots(blk)
    v = np.zeros_like(blk)
    v[sl] = blk[sl] * np.random.default_rng(3).standard_normal(len(sl))  # a direction in log-parameter space
    d0 = float(g0["block"].numpy() @ v)
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), kernel="composite", jitter=1e-6, engine=engine)
    assert not cb._small_ok(M) and cb._whitened(M)
    F1, g1 = cb.value_and_grad(Z.to(engine.device), blk.tolist(), 1.0, s2)
    cb.factored_adjoint = False
    F2, g2 = cb.value_and_grad(Z.to(engine.device), blk.tolist(), 1.0, s2)
    assert abs(F1 - float(F0)) < 1e-8 * abs(float(F0)) and F1 == F2
    e1 = abs(float(g1["ls"].numpy() @ v) - d0) / abs(d0)
    e2 = abs(float(g2["ls"].numpy() @ v) - d0) / abs(d0)
    print("directional derivative, relative error: factored %.2e, explicit Phibar %.2e" % (e1, e2))
    assert e1 < 2e-4, (e1, e2)          # (the oracle's own autograd is good to ~1e-5 here)
    assert e2 > 10 * e1                 # what the factored form is for
    assert abs(g1["s2"] - float(g0["s2"])) < 1e-5 * abs(float(g0["s2"]))


@pytest.mark.gpu
def test_factored_pass2_matches_explicit_on_well_conditioned_problems(engine):
    """Same gradients from both forms of pass 2 where Phibar is harmless: stationary kernels (d = 3 and d = 18 -> the kernel's
    one-pass epilogue without the K'_fu re-read) and a composite one, incl. dF/dZ, M above the single-launch limit."""
    import ggp_amd
    g = torch.Generator().manual_seed(12)
    for (N, d, M, kern) in [(900, 3, 150, "rbf"), (700, 18, 130, "rbf"), (800, 2, 140, "matern32"), (600, 1, 160, "composite")]:
        X = torch.rand(N, d, dtype=torch.float64, generator=g) * (40.0 if kern == "composite" else 6.0)
        y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
        Z = X[torch.randperm(N, generator=g)[:M]].clone()
        cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), kernel=kern, jitter=1e-6, engine=engine, form="whitened")
        if kern == "composite":
            ls, sf2 = CO.make_block([(1.1, [(CO.PERIODIC, 1.2, 6.3), (CO.EXPQUAD, 20.0)]), (0.3, [(CO.MATERN32, 0.8)])]).tolist(), 1.0
        else:
            ls, sf2 = [1.5] * d, 1.3
        Fa, ga = cb.value_and_grad(Z.to(engine.device), ls, sf2, 0.05, want_gz=True)
        cb.factored_adjoint = False
        Fb, gb = cb.value_and_grad(Z.to(engine.device), ls, sf2, 0.05, want_gz=True)
        assert Fa == Fb
        sc = max(1.0, float(gb["ls"].abs().max()))
        assert float((ga["ls"] - gb["ls"]).abs().max()) < 1e-8 * sc, (kern, d)
        assert abs(ga["sf2"] - gb["sf2"]) < 1e-8 * max(1.0, abs(gb["sf2"])) and abs(ga["s2"] - gb["s2"]) < 1e-8 * max(1.0, abs(gb["s2"]))
        assert float((ga["Z"] - gb["Z"]).abs().max()) < 1e-8 * max(1.0, float(gb["Z"].abs().max())), (kern, d)
