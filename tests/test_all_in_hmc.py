"""all_in_HMC on the CPU (the wide header's sanitizer build: tests/test_all_in_hmc_sanitizers.py): the joint target (theta AND the inducing inputs) over the oracle-backed test double against an autograd
yardstick, the wide device sampler (csrc/sgp_nuts_wide.hpp) compiled for the host against hmc.NUTS, and the model class with
its per-draw-Z mixture predictive end to end."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from fake_engine import OracleEngine
from oracle import vfe_oracle as O

import ggp_amd
from ggp_amd.hmc import NUTS, DiagMassAdapter, SplitMix

INC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "nuts_wide_host.cpp")


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def yardstick(X, y, M, d, q):
    """oracle.vfe_pymc3_order + the theta priors / Jacobians + Z ~ Normal(0, 1); gradient over (theta, Z) by autograd."""
    qt = torch.tensor(np.asarray(q, dtype=np.float64), requires_grad=True)
    ls, sf, sn = torch.exp(qt[:d]), torch.exp(qt[d]), torch.exp(qt[d + 1])
    Z = qt[d + 2:].reshape(M, d)
    F = O.vfe_pymc3_order(T(X), T(y).reshape(-1), Z, ls, sf, sn, jitter=1e-6)
    c = math.log(2.0) - math.log(math.pi)
    lp = F + torch.sum(torch.log(ls) - ls) + (c - torch.log1p(sf * sf)) + (c - torch.log1p(sn * sn)) + torch.sum(qt[:d + 2])
    lp = lp - 0.5 * torch.sum(Z * Z) - 0.5 * math.log(2.0 * math.pi) * M * d
    lp.backward()
    return float(lp.detach()), qt.grad.numpy().copy()


def joint_target(X, y, M):
    cb = ggp_amd.CollapsedBound(T(X), T(y).reshape(-1), jitter=1e-6, engine=OracleEngine())
    return ggp_amd.JointHmcTarget(cb, M)


@pytest.mark.parametrize("name", ["rbf_d1_tiny", "rbf_d3_small"])
def test_joint_target_matches_the_yardstick(name):
    G = load_golden(name)
    M, d = np.asarray(G["Z"]).shape
    tgt = joint_target(G["X"], G["y"], M)
    assert tgt.ndim == d + 2 + M * d and not tgt.device_sampler_ok()
    q = np.concatenate([np.log(np.asarray(G["ls"], dtype=np.float64).reshape(-1)) + 0.1,
                        [0.5 * math.log(float(G["sf2"])), 0.5 * math.log(float(G["s2"])) - 0.1], np.asarray(G["Z"]).reshape(-1)])
    lp, g = tgt.logp_and_grad(q)
    lp_ref, g_ref = yardstick(G["X"], G["y"], M, d, q)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    assert np.allclose(g, g_ref, rtol=1e-7, atol=1e-7 * np.max(np.abs(g_ref)))
    # central differences at a few entries: theta and Z
    for i in (0, d + 1, d + 2, len(q) - 1):
        h = 1e-5
        qp, qm = q.copy(), q.copy()
        qp[i] += h
        qm[i] -= h
        fd = (tgt.logp(qp) - tgt.logp(qm)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-5 * max(1.0, abs(g[i]))
    # the PyMC3 test point and the constrained view
    assert tgt.start()[d + 2:] == [0.0] * (M * d)
    c = tgt.constrain(q)
    assert c["Z"].shape == (M, d) and np.array_equal(c["Z"].reshape(-1), q[d + 2:])
    # out of range: -inf, never an exception
    bad = q.copy()
    bad[0] = 400.0
    assert tgt.logp_and_grad(bad)[0] == -math.inf


# ---- the wide sampler's host build ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("wide") / "libnuts_wide_host.so")
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", INC, "-o", so, SRC], check=True, timeout=300)
    lib = C.CDLL(so)
    lib.nuts_wide_host_run.restype = C.c_long
    lib.nuts_wide_host_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_ulonglong,
                                       C.POINTER(C.c_double), CB, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    return lib


CB = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run_wide(lib, f, nd, q0, tune, draws, seed, depth):
    def cb(qp, lpp, gp):
        lp, g = f(np.ctypeslib.as_array(qp, (nd,)).copy())
        lpp[0] = lp
        np.ctypeslib.as_array(gp, (nd,))[:] = g
    q0 = np.ascontiguousarray(q0, dtype=np.float64)
    S, St = np.zeros((draws, nd)), np.zeros((draws, 8))
    nl = lib.nuts_wide_host_run(nd, tune, draws, depth, 0.25, 0.8, seed, _p(q0), CB(cb), _p(S), _p(St))
    assert nl >= 0, "the slot pool did not come back to the current state alone"
    return S, St, nl


def fixed_order_dot(a, b):
    """The reduction order of csrc/sgp_nuts_wide.hpp: lane t sums entries t, t + 256, ... in order; each wave of 64 lanes folds
    v[t] += v[t + h], h = 32 ... 1; the four wave sums combine as (w0 + w1) + (w2 + w3)."""
    x = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    k = -(-x.size // 256)
    pad = np.zeros(k * 256)
    pad[:x.size] = x
    lanes = np.zeros(256)
    for r in range(k):
        lanes = lanes + pad[r * 256:(r + 1) * 256]
    w = lanes.reshape(4, 64).copy()
    h = 32
    while h >= 1:
        w[:, :h] = w[:, :h] + w[:, h:2 * h]
        h //= 2
    return float((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))


class FixedOrderNUTS(NUTS):
    _dot = staticmethod(fixed_order_dot)


def run_python(f, nd, q0, tune, draws, seed, depth):
    nuts = FixedOrderNUTS(f, nd, max_treedepth=depth, rng=SplitMix(seed))
    q = np.array(q0, dtype=np.float64)
    lp, g = nuts._eval(q)
    nuts.mass = DiagMassAdapter(nd, initial_mean=q)
    S, St = [], []
    for it in range(tune + draws):
        q, lp, g, st = nuts.draw(q, lp, g, it < tune)
        if it >= tune:
            S.append(q.copy())
            St.append([st["step_size"], st["tree_size"], st["depth"], st["mean_tree_accept"], float(st["diverging"]), st["energy"], lp,
                       nuts.n_leapfrog])
    return np.array(S), np.array(St), nuts.n_leapfrog


def _same_chain(a, b, rtol=1e-10, atol=1e-12):
    assert a[2] == b[2], "leapfrog counts differ: the trees differ"
    assert np.array_equal(a[1][:, 1:3], b[1][:, 1:3])  # tree sizes, depths
    assert np.array_equal(a[1][:, 4], b[1][:, 4])      # divergences
    assert np.allclose(a[1][:, 0], b[1][:, 0], rtol=1e-10, atol=0)
    assert np.allclose(a[0], b[0], rtol=rtol, atol=atol)


@pytest.mark.parametrize("nd", [40, 700, 3098])
def test_wide_sampler_equals_the_python_sampler_on_a_gaussian(wide_lib, nd):
    rng = np.random.default_rng(nd)
    mu = rng.standard_normal(nd)
    sd = np.exp(rng.uniform(-1.5, 1.0, nd))

    def f(q):
        z = (q - mu) / sd
        return float(-0.5 * np.sum(z * z)), -z / sd

    q0 = mu + 0.3
    # bit-identical at 40 and 700; at 3 098 the chains part by ~1e-10 (absolute, entries of order 1) during tuning
    _same_chain(run_wide(wide_lib, f, nd, q0, 20, 15, 17, 6), run_python(f, nd, q0, 20, 15, 17, 6), 
                **({} if nd < 1000 else {"rtol": 1e-9, "atol": 1e-9}))


def test_wide_sampler_handles_divergences_alike(wide_lib):
    def f(q):
        if q[0] > 1.2:
            return -math.inf, np.zeros_like(q)
        s = np.linspace(0.1, 2.0, q.size)
        return float(-0.5 * np.sum((q / s) ** 2)), -q / s ** 2

    _same_chain(run_wide(wide_lib, f, 300, np.full(300, 0.2), 25, 20, 9, 8), run_python(f, 300, np.full(300, 0.2), 25, 20, 9, 8))


def test_wide_sampler_on_the_joint_target(wide_lib):
    """The joint target at M = 4, d = 2 (oracle-backed engine): the same chain from both samplers."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 2))
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(40)
    tgt = joint_target(X, y, 4)
    q0 = np.array(tgt.start()) + SplitMix(5).uniform(-1.0, 1.0, tgt.ndim)
    _same_chain(run_wide(wide_lib, tgt.logp_and_grad, tgt.ndim, q0, 20, 15, 23, 6),
                run_python(tgt.logp_and_grad, tgt.ndim, q0, 20, 15, 23, 6))


# ---- the model class ------------------------------------------------------------------------------------------------
def _model(M=5, d=2, N=40, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(N)
    m = ggp_amd.all_in_HMC(T(X), T(y), ggp_amd.GaussianLikelihood(), T(X[:M]), engine=OracleEngine(), seed=seed)
    return m, X, y


def test_all_in_hmc_train_model_and_trace():
    m, X, y = _model()
    m.sample = (lambda f: (lambda n, dim, tune: f(6, dim, 10)))(m.sample)  # the reference's 500 + 100, shortened
    tr, steps, perf = m.train_model()
    assert len(tr) == 6 and len(steps) == 1 and len(perf) == 1 and steps[0] > 0.0
    assert tr['Z'].shape == (6, 5, 2) and tr[0]['Z'].shape == (5, 2)
    assert tr['ls'].shape == (6, 2) and np.all(np.isfinite(tr.get_sampler_stats('logp')))
    assert np.array_equal(tr[3]['theta_unc'][4:].reshape(5, 2), tr[3]['Z'])


def test_full_mixture_predictive_uses_each_draws_z(capsys):
    m, X, y = _model()
    tr = m.sample(4, 2, 8)
    rng = np.random.default_rng(0)
    Xs = rng.standard_normal((7, 2))
    tr[1]['sig_n'] = 0.005  # below the noise floor: becomes 0.01
    tr[2]['ls'] = np.full(2, np.nan)  # a broken draw: its predictive fails the PSD gate and is skipped
    preds = ggp_amd.full_mixture_posterior_predictive(m, T(Xs), tr)
    out = capsys.readouterr().out
    assert tr[1]['sig_n'] == 0.01
    assert 'Not psd for sample 2' in out
    kept = [i for i in range(4) if ('Not psd for sample %d' % i) not in out]
    assert len(preds) == len(kept)
    for p, i in zip(preds, kept):
        h = tr[i]
        ref_mu, ref_var = O.predict(T(Xs), T(X), T(y), T(h['Z']), T(h['ls']), h['sig_f'] ** 2, h['sig_n'] ** 2, jitter=0.0)[:2]
        assert np.allclose(p.mean.detach().numpy(), ref_mu.numpy(), rtol=1e-9, atol=1e-10)
        assert np.allclose(p.variance.detach().numpy(), ref_var.numpy(), rtol=1e-9, atol=1e-10)
    assert np.array_equal(m.covar_module.inducing_points.data.numpy(), tr[3]['Z'])


# ---- exact posterior of a tiny joint problem ------------------------------------------------------------------------
def _vfe_m1(X, y, ls, sf, sn, z):
    """Closed-form VFE bound for M = 1, d = 1 (Kuu = sf^2 + 1e-6, a rank-one Q), vectorised over grids of (ls, sf, sn, z)."""
    N = X.size
    sf2, s2 = sf * sf, sn * sn
    kuu = sf2 + 1e-6
    r = (X[(None,) * ls.ndim] - z[..., None]) / ls[..., None]
    k = sf2[..., None] * np.exp(-0.5 * r * r)
    kk, ky = np.sum(k * k, -1), np.sum(k * y, -1)
    den = kuu * s2 + kk
    logdet = N * np.log(s2) + np.log(den / (kuu * s2))
    quad = (float(y @ y) - ky * ky / den) / s2
    trace = (N * sf2 - kk / kuu) / (2.0 * s2)
    return -0.5 * N * math.log(2.0 * math.pi) - 0.5 * logdet - 0.5 * quad - trace


def _ess(x):
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    c = x - x.mean()
    f = np.fft.rfft(c, 2 * n)
    rho = np.fft.irfft(f * np.conj(f))[:n]
    rho = rho / rho[0]
    s = 0.0
    for k in range(0, n - 1, 2):
        if rho[k] + rho[k + 1] < 0.0:
            break
        s += rho[k] + rho[k + 1]
    return n / max(2.0 * s - 1.0, 1.0 / n)


def test_joint_nuts_lands_on_the_exact_posterior():
    """M = 1, d = 1, six data points (ndim 4): posterior means by quadrature on a 4-D grid of the closed-form density above;
    host-driven joint NUTS (JointHmcTarget over the oracle-backed engine) within 4 Monte-Carlo standard errors of every mean."""
    X = np.array([-1.5, -0.7, 0.1, 0.6, 1.2, 1.9])
    y = np.array([-0.9, -0.5, 0.2, 0.5, 0.8, 1.1])
    # the closed form against the target itself at one point
    tgt = joint_target(X[:, None], y, 1)
    q = np.array([0.3, -0.2, -1.1, 0.4])
    lp = tgt.logp(q)
    c = math.log(2.0) - math.log(math.pi)
    ls, sf, sn, z = np.exp(q[0]), np.exp(q[1]), np.exp(q[2]), q[3]
    ref = (_vfe_m1(X, y, np.array(ls), np.array(sf), np.array(sn), np.array(z)) + math.log(ls) - ls + (c - math.log1p(sf * sf))
           + (c - math.log1p(sn * sn)) + q[:3].sum() - 0.5 * z * z - 0.5 * math.log(2.0 * math.pi))
    assert abs(lp - float(ref)) <= 1e-10 * abs(lp)
    # quadrature: logp on a grid over the unconstrained space (mass at the edges checked below)
    axes = [np.linspace(-4.0, 4.5, 40), np.linspace(-11.0, 5.5, 56), np.linspace(-8.0, 2.0, 40), np.linspace(-6.0, 6.0, 44)]
    A, B, Cg, D = np.meshgrid(*axes, indexing="ij")
    ls, sf, sn = np.exp(A), np.exp(B), np.exp(Cg)
    logp = (_vfe_m1(X, y, ls, sf, sn, D) + np.log(ls) - ls + (c - np.log1p(sf * sf)) + (c - np.log1p(sn * sn)) + A + B + Cg
            - 0.5 * D * D)
    w = np.exp(logp - logp.max())
    w /= w.sum()
    for ax in range(4):
        marg = w.sum(axis=tuple(k for k in range(4) if k != ax))
        assert marg[0] < 1e-4 and marg[-1] < 1e-4, ("the grid must hold the posterior", ax, marg[0], marg[-1])
    exact = np.array([np.sum(w * G) for G in (A, B, Cg, D)])
    sd = np.sqrt(np.array([np.sum(w * G * G) for G in (A, B, Cg, D)]) - exact ** 2)
    tr = ggp_amd.sample_nuts(tgt, 1500, 300, seed=11)
    draws = np.stack([r["theta_unc"] for r in tr])
    for k in range(4):
        mcse = draws[:, k].std() / math.sqrt(_ess(draws[:, k]))
        assert abs(draws[:, k].mean() - exact[k]) < 4.0 * mcse, (k, draws[:, k].mean(), exact[k], mcse, sd[k])
