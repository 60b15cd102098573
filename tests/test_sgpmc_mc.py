"""CPU: ``SgpmcTarget(likelihood="multiclass")`` over the CPU double (tests/sgpmc_mc_double.py) against central differences of its own
``logp``, the label checks, ``ndim`` / ``constrain``, ``likelihood_moments("multiclass")`` and ``predict_sgpmc``, the 1-D demo's record,
and the lengths of the two new prototypes."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import ggp_amd
from ggp_amd.sgp_hmc import likelihood_moments
from sgpmc_mc_double import SgpmcMcOracleEngine, class_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The demo on the CPU double with DEMO_KW (measured here, float64): held-out accuracy 0.85 against a majority-class frequency of 0.32,
# mean log predictive probability -0.716 against log(1/3) = -1.099.  The test asserts the two baselines, not these numbers.
DEMO_KW = dict(seed=3, tune=40, num_samples=40, warmup_iters=40, n_draws=40)
DEMO_CPU = {"accuracy": 0.85, "mean_log_pred_prob": -0.716}


def demo_module():
    spec = importlib.util.spec_from_file_location("demo_1d_classification", os.path.join(ROOT, "experiments", "demo_1d_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problem(N=40, M=6, d=2, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, d))
    Z = rng.uniform(-2.0, 2.0, (M, d))
    X[:2] = Z[:2]                                  # data on inducing inputs
    f = np.stack([np.sin(2 * X[:, 0]), np.cos(2 * X[:, 1]), 0.3 * X[:, 0] * X[:, 1]], 1)
    y = np.argmax(f + 0.3 * rng.standard_normal((N, 3)), 1).astype(np.float64)
    return torch.as_tensor(X), torch.as_tensor(y), torch.as_tensor(Z)


@pytest.mark.parametrize("num_classes", [None, 4])
def test_logp_and_grad_against_central_differences(num_classes):
    X, y, Z = problem()
    t = ggp_amd.SgpmcTarget(X, y, Z, engine=SgpmcMcOracleEngine(), likelihood="multiclass", num_classes=num_classes)
    Cn, M, d = num_classes or 3, 6, 2
    assert t.num_classes == Cn and t.ndim == d + 1 + M * Cn and len(t.start()) == t.ndim
    c = t.constrain(t.start())
    assert c["V"].shape == (Cn, M) and "noise_variance" not in c and len(c["lengthscales"]) == d
    rng = np.random.default_rng(7)
    for vs in (0.0, 1.0, 3.0):
        q = np.concatenate([np.asarray(t.start()[:1 + d]) + 0.3 * rng.standard_normal(1 + d), vs * rng.standard_normal(M * Cn)])
        lp, g, gz = t.logp_and_grad(q, want_gz=True)
        assert t.logp(q) == pytest.approx(lp, rel=1e-13)
        h = 1e-6
        fd = np.array([(t.logp(q + h * e) - t.logp(q - h * e)) / (2 * h) for e in np.eye(len(q))])
        # central differences of a smooth float64 function with |F| ~ 1e2: truncation h^2 |F'''| ~ 1e-10 and rounding eps |F| / h ~ 1e-8
        assert np.abs(fd - np.asarray(g)).max() <= 1e-6 * (1.0 + np.abs(fd).max())
        Z0 = t.Z.clone()
        fdz = np.zeros((M, d))
        for i in range(M):
            for j in range(d):
                for s in (1.0, -1.0):
                    Zs = Z0.clone()
                    Zs[i, j] += s * h
                    t.set_Z(Zs)
                    fdz[i, j] += s * t.logp(q) / (2 * h)
        t.set_Z(Z0)
        assert np.abs(fdz - gz.numpy()).max() <= 1e-6 * (1.0 + np.abs(fdz).max())
    assert t.engine.calls["sgpmc_mc_rows"] == t.engine.calls["sgpmc_mc_tail"] and t.engine.calls["sgpmc_lik_rows"] == 0
    assert t.last_pass1 == "sgpmc_mc_rows"


def test_bad_labels_and_class_counts_raise():
    X, y, Z = problem()
    mk = lambda yy, **kw: ggp_amd.SgpmcTarget(X, yy, Z, engine=SgpmcMcOracleEngine(), likelihood="multiclass", **kw)
    for bad in (y + 0.5, -y - 1.0, torch.where(y == 0, torch.full_like(y, float("nan")), y)):
        with pytest.raises(ValueError):
            mk(bad)
    with pytest.raises(ValueError):
        mk(y, num_classes=2)                        # the labels reach 2
    with pytest.raises(ValueError):
        mk(y, num_classes=17)
    with pytest.raises(ValueError):
        mk(torch.zeros_like(y))                     # one class only: C = 1
    with pytest.raises(ValueError):
        mk(y, num_classes=3.5)
    with pytest.raises(ValueError):
        mk(y, robustmax_eps=0.0)
    with pytest.raises(ValueError):
        ggp_amd.SgpmcTarget(X, y, Z, engine=SgpmcMcOracleEngine(), likelihood="poisson", num_classes=3)
    assert mk(torch.zeros_like(y), num_classes=2).num_classes == 2


def test_class_probabilities_of_the_host_step():
    rng = np.random.default_rng(2)
    mu, var = rng.standard_normal((7, 5, 4)) * 2.0, rng.uniform(0.05, 3.0, (7, 5))
    p, sd = likelihood_moments("multiclass", mu, var)
    assert p.shape == sd.shape == (7, 5, 4) and np.allclose(sd, np.sqrt(p * (1 - p)))
    # the probabilities of "c is the largest" sum to one up to the 20-point rule's error on a product of three Phi's
    assert np.abs(p.sum(-1) - 1.0).max() < 1e-4
    ref = class_probs(torch.as_tensor(mu.reshape(-1, 4)), torch.as_tensor(var.reshape(-1)), 1e-3).numpy().reshape(7, 5, 4)
    assert np.abs(p - ref).max() < 1e-14
    # ties: every class the same
    p0, _ = likelihood_moments("multiclass", np.zeros((3, 4)), np.ones(3))
    assert np.abs(p0 - 0.25).max() < 1e-6
    # a clear winner: 1 - eps for it, eps / (C - 1) for the others
    p1, _ = likelihood_moments("multiclass", np.array([[40.0, 0.0, -3.0]]), np.array([0.5]), eps=1e-2)
    assert np.allclose(p1, [[0.99, 0.005, 0.005]], atol=1e-12)


@pytest.fixture(scope="module")
def demo_run():
    demo = demo_module()
    return demo, demo.run(SgpmcMcOracleEngine(), **DEMO_KW)


def test_demo_record_clears_both_baselines(demo_run):
    demo, r = demo_run
    print("SGPMC_MC demo on the CPU double:", {k: r[k] for k in ("accuracy", "mean_log_pred_prob", "baseline_majority_accuracy")})
    assert r["classes"] == 3 and r["N_train"] == 40 and r["N_test"] == 160 and r["n_mixture"] == 40
    assert r["mean_log_pred_prob"] > r["baseline_log_uniform"] == pytest.approx(np.log(1.0 / 3.0))
    assert r["accuracy"] > r["baseline_majority_accuracy"]
    assert r["warmup"]["loss_end"] < r["warmup"]["loss_start"] and 0.0 < r["acceptance"] <= 1.0
    Xtr, ytr, Xte, yte = demo.make_data(3)
    assert Xtr.shape == (40,) and Xte.shape == (160,) and set(np.unique(np.concatenate([ytr, yte]))) == {0.0, 1.0, 2.0}
    assert 0.0 <= Xtr.min() and Xtr.max() <= 10.0 and not set(Xtr) & set(Xte)


def test_predict_sgpmc_shapes_and_probabilities():
    X, y, Z = problem(N=30, M=5, d=2)
    X, Z = X[:, :1].contiguous(), Z[:, :1].contiguous()            # one input dimension (the labels still come from two)
    model, trace, _ = ggp_amd.train_sgp_hmc((X, y), Z, 1, 5, 6, engine=SgpmcMcOracleEngine(), seed=1, warmup_iters=3, likelihood="multiclass")
    assert model.likelihood == "multiclass" and model.target.num_classes == 3 and np.asarray(trace[0]["V"]).shape == (3, 5)
    Xs = torch.linspace(-2.0, 2.0, 11, dtype=torch.float64)
    mean, probs, sd = ggp_amd.predict_sgpmc(model, trace, Xs, n_draws=4)
    assert mean.shape == (11, 3) and probs.shape == sd.shape == (4, 11, 3)
    assert np.abs(probs.sum(-1) - 1.0).max() < 1e-4 and np.allclose(mean, probs.mean(0)) and (probs > 0).all()


def test_prototypes_and_constants():
    from ggp_amd import _lib
    assert _lib.SGP_LIK_MULTICLASS_ROBUSTMAX == 4 and _lib.SGP_MAX_CLASSES == 16 and max(_lib.LIKELIHOOD_IDS.values()) == 3
    assert len(_lib.PROTOTYPES["sgp_sgpmc_mc_rows"][1]) == 27 and len(_lib.PROTOTYPES["sgp_sgpmc_mc_tail"][1]) == 16
    hdr = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert "#define SGP_LIK_MULTICLASS_ROBUSTMAX 4" in hdr and "#define SGP_MAX_CLASSES 16" in hdr and "#define SGP_ABI_VERSION 3" in hdr
