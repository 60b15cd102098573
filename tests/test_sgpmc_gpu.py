"""GPU: the SGPMC tail (csrc/sgp_sgpmc.hip) through the C ABI against the long-double reference, ``SgpmcTarget`` / ``sample_hmc`` /
``predict_sgpmc`` on the device against the CPU double.  The argument checks of the new entry point need no GPU and run everywhere."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import dev

import ggp_amd
import pass2_reference as P2
import sgpmc_reference as R
from sgpmc_double import SgpmcOracleEngine

T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
OUT_KEYS = ("F", "data", "prior", "s2bar", "kappabar")


def f64(a):
    return np.asarray(a, dtype=np.float64)


def padded_linv(Li, M):
    Mp = (M + 127) // 128 * 128
    P = np.eye(Mp)
    P[:M, :M] = f64(Li)
    return P


def call_tail(engine, ref, yy, kappa, v, s2, N, with_adj, ws=None):
    """sgp_sgpmc_from_whitened_stats on the fp64 images of the reference's whitened inputs; every output as numpy."""
    M = v.shape[0]
    lib = engine.lib
    W, u, vv = dev(f64(ref["W"]), engine), dev(f64(ref["u"]), engine), dev(v, engine)
    sc = dev(np.array([float(yy), float(kappa)]), engine)
    linv = dev(padded_linv(ref["Linv"], M), engine)
    nan = float("nan")
    out = torch.full((5,), nan, dtype=torch.float64, device=engine.device)
    vbar, bbar = (torch.full((M,), nan, dtype=torch.float64, device=engine.device) for _ in range(2))
    Cw, Kuubar = (torch.full((M, M), nan, dtype=torch.float64, device=engine.device) for _ in range(2))
    nbytes = lib.sgp_sgpmc_workspace_bytes(M)
    assert nbytes > 0
    if ws is None:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=engine.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    st = lib.sgp_sgpmc_from_whitened_stats(p(W), p(u), C.c_void_p(sc.data_ptr()), C.c_void_p(sc.data_ptr() + 8), p(vv), float(s2), int(N), M,
                                           1 if with_adj else 0, p(out), p(vbar) if with_adj else null, p(Cw) if with_adj else null,
                                           p(bbar) if with_adj else null, p(Kuubar) if with_adj else null, p(linv) if with_adj else null,
                                           p(ws), ws.numel(), null)
    assert st == 0
    torch.cuda.synchronize()
    got = dict(zip(OUT_KEYS, out.cpu().numpy()))
    if with_adj:
        got.update(vbar=vbar.cpu().numpy(), Cw=Cw.cpu().numpy(), bbar=bbar.cpu().numpy(), Kuubar=Kuubar.cpu().numpy())
    return got


def tail_problem(M, seed, spacing=None):
    """(K, Phi, b, yy, kappa, N, s2) in long double.  spacing: inducing inputs on a line, that fraction of a lengthscale apart, with the
    jitter that puts cond(K_uu) at 1e8."""
    rng = np.random.default_rng(seed)
    N, d = 50, 2
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    ls, sf2, s2, jitter = np.array([1.1, 0.8]), 1.3, 0.15, 1e-5
    if spacing is None:
        Z = 1.5 * rng.standard_normal((M, d))
    else:
        Z = np.stack([spacing * ls[0] * np.arange(M), np.zeros(M)], 1) - 1.0
        K0 = R.kernel_blocks(X, y, Z, ls, sf2, 0.0, 0)[0]
        jitter = float(np.linalg.eigvalsh(f64(K0)).max()) / 1e8
    K, Phi, b, yy, kappa = R.kernel_blocks(X, y, Z, ls, sf2, jitter, 0)
    return K, Phi, b, yy, kappa, N, s2


def check_tail(engine, prob, vs):
    K, Phi, b, yy, kappa, N, s2 = prob
    M = K.shape[0]
    worst = 0.0
    for v in vs:
        ref, A = R.reference(K, Phi, b, yy, kappa, v, s2, N)
        full = call_tail(engine, ref, yy, kappa, v, s2, N, True)
        for k in OUT_KEYS + ("vbar", "Cw", "bbar", "Kuubar"):
            worst = max(worst, P2.assert_close(full[k], ref[k], A[k], what="M=%d %s" % (M, k)))
        value = call_tail(engine, ref, yy, kappa, v, s2, N, False)
        for k in OUT_KEYS:   # the value-only call: the same bits
            assert value[k] == full[k], (M, k)
        # a NaN-poisoned workspace and a second call: bit-equal results
        ws = torch.full((engine.lib.sgp_sgpmc_workspace_bytes(M) // 8,), float("nan"), dtype=torch.float64, device=engine.device).view(torch.uint8)
        again = call_tail(engine, ref, yy, kappa, v, s2, N, True, ws=ws)
        for k in full:
            assert np.array_equal(again[k], full[k]), (M, k, "poisoned workspace")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5, 64, 65, 129, 200])
def test_tail_against_the_long_double_reference(engine, M):
    """|got - ref| <= 1e-12 A for every output (the rule and constant of tests/test_pass2_kernel.py), v = 0, standard normal and
    30 x standard normal, with and without the adjoints."""
    rng = np.random.default_rng(100 + M)
    z = rng.standard_normal(M)
    worst = check_tail(engine, tail_problem(M, M), [np.zeros(M), z, 30.0 * z])
    print("M = %d: worst |got - ref| / A = %.3e" % (M, worst))


@pytest.mark.gpu
def test_tail_at_cond_1e8(engine):
    M = 24
    prob = tail_problem(M, 7, spacing=0.1)
    cond = np.linalg.cond(f64(prob[0]))
    assert 3e7 < cond < 3e8, cond
    worst = check_tail(engine, prob, [np.random.default_rng(8).standard_normal(M)])
    print("cond(K_uu) = %.2e: worst |got - ref| / A = %.3e" % (cond, worst))


def test_bad_arguments_are_rejected_before_any_launch():
    """SGP_ERR_ARG before SGP_ERR_DIM before SGP_ERR_WORKSPACE, on dummy pointers that are never dereferenced."""
    import __graft_entry__ as ge
    ge.build()
    lib = ggp_amd.load_library()
    one, null = C.c_void_p(8), C.c_void_p(0)
    big = 1 << 40

    def call(W=one, u=one, yy=one, kappa=one, v=one, s2=0.1, N=10, M=4, adj=1, out=one, vbar=one, Cw=one, bbar=one, Kuubar=one, linv=one,
             ws=null, nbytes=0):
        return lib.sgp_sgpmc_from_whitened_stats(W, u, yy, kappa, v, s2, N, M, adj, out, vbar, Cw, bbar, Kuubar, linv, ws, nbytes, null)

    for name in ("W", "u", "yy", "kappa", "v", "out", "vbar", "Cw", "bbar", "Kuubar", "linv"):
        assert call(**{name: null}) == -1, name
    assert call(s2=0.0) == -1 and call(s2=-1.0) == -1 and call(s2=float("nan")) == -1 and call(M=0) == -1 and call(N=-1) == -1
    assert call(M=4097) == -2 and call(M=4097, W=null) == -1 and call(M=4097, ws=one, nbytes=big) == -2
    assert call() == -3 and call(ws=one, nbytes=1) == -3 and call(ws=null, nbytes=big) == -3
    assert call(adj=0, vbar=null, Cw=null, bbar=null, Kuubar=null, linv=null) == -3      # valid without the adjoints, except for its workspace
    assert lib.sgp_sgpmc_workspace_bytes(0) == 0 and lib.sgp_sgpmc_workspace_bytes(4097) == 0
    assert 0 < lib.sgp_sgpmc_workspace_bytes(1) == lib.sgp_sgpmc_workspace_bytes(128) < lib.sgp_sgpmc_workspace_bytes(129)


# ---------------------------------------------------------------------------------------------
# the target on the device against the CPU double
# ---------------------------------------------------------------------------------------------
def target_problem(N, M, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    Z = X[rng.choice(N, M, replace=False)] + 0.05 * rng.standard_normal((M, d)) if M <= N else rng.standard_normal((M, d))
    return X, y, Z


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,d,kernel", [(1, 1, 1, "rbf"), (37, 5, 1, "rbf"), (300, 65, 3, "rbf"), (300, 65, 3, "matern52"), (5000, 129, 3, "rbf")])
def test_target_on_the_device_against_the_cpu_double(engine, N, M, d, kernel):
    X, y, Z = target_problem(N, M, d, N + M)
    gpu = ggp_amd.SgpmcTarget(dev(X, engine), dev(y, engine), dev(Z, engine), kernel=kernel, engine=engine)
    cpu = ggp_amd.SgpmcTarget(T(X), T(y), T(Z), kernel=kernel, engine=SgpmcOracleEngine())
    rows = N * M >= 5000 * 129
    if rows:   # the streaming layout of the whitened pass 1 (what a C5-sized shard takes), at a size a test can afford
        gpu.whitened_rows_min_work = cpu.whitened_rows_min_work = N * M
    rng = np.random.default_rng(5)
    q = np.asarray(gpu.start()) + np.concatenate([rng.uniform(-0.3, 0.3, d + 2), 0.5 * rng.standard_normal(M)])
    lp_ref, g_ref, gz_ref = cpu.logp_and_grad(q, want_gz=True)
    g_ref = np.asarray(g_ref)
    for want_gz in (False, True):
        r = gpu.logp_and_grad(q, want_gz=want_gz)
        assert gpu.last_pass1 == ("suffstats_whitened_rows" if rows else "suffstats_whitened")
        assert len(r) == (3 if want_gz else 2)
        assert abs(r[0] - lp_ref) <= 1e-8 * N, (r[0], lp_ref)
        assert np.abs(np.asarray(r[1]) - g_ref).max() <= 1e-6 * np.abs(g_ref).max()
        if want_gz:
            assert float((r[2].cpu() - gz_ref).abs().max()) <= 1e-6 * float(gz_ref.abs().max())
    assert abs(gpu.logp(q) - lp_ref) <= 1e-8 * N


@pytest.mark.gpu
def test_marginal_identity_on_the_device(engine):
    """F(m) + M/2 log 2 pi - 1/2 log det B = the collapsed bound in the whitened order at the same theta and jitter, with m from a host
    solve of the device's own W and u."""
    N, M, d = 300, 65, 3
    X, y, Z = target_problem(N, M, d, 11)
    Xd, yd, Zd = dev(X, engine), dev(y, engine), dev(Z, engine)
    ls, sf2, s2, jitter = [0.9, 1.3, 1.1], 1.2, 0.08, 1e-5
    result = engine.result_buffer()
    Kuu = engine.kuu(Zd, ls, sf2, jitter, "rbf")
    linv, _ = engine.kuu_factor(Kuu, info=result[2])
    packed = engine.suffstats_whitened(Xd, yd, Zd, ls, sf2, linv, "rbf")
    h = packed.cpu()
    W, u = h[:M * M].reshape(M, M), h[M * M:M * M + M]
    B = torch.eye(M, dtype=torch.float64) + 0.5 * (W + W.T) / s2
    m = torch.linalg.solve(B, u) / s2
    res = engine.sgpmc_tail(packed, m.to(engine.device), s2, N, linv, with_adjoints=True, result=result)
    o, info = engine.read_result(res["buf"].cpu())
    assert info == 0
    marg = o[0] + 0.5 * M * math.log(2.0 * math.pi) - 0.5 * float(torch.linalg.slogdet(B)[1])
    F = ggp_amd.CollapsedBound(Xd, yd, jitter=jitter, engine=engine, form="whitened").value(Zd, ls, sf2, s2)[0]
    assert abs(marg - F) <= 1e-8 * N, (marg, F)
    assert float(res["vbar"].abs().max()) <= 1e-8 * N


def sampler_problem():
    rng = np.random.default_rng(2)
    X = np.sort(rng.uniform(-3.0, 3.0, 60))[:, None]
    y = np.sin(2.0 * X[:, 0]) + 0.2 * rng.standard_normal(60)
    return X, y, np.linspace(-2.5, 2.5, 6)[:, None]


@pytest.mark.gpu
def test_same_seed_same_chain_on_the_device_and_over_the_double(engine):
    """N = 60, M = 6: twenty transitions (ten of them adapting the step; no burn-in, so that the trace shows all twenty) agree to 1e-6
    and take the same accept decisions."""
    X, y, Z = sampler_problem()
    gpu = ggp_amd.SgpmcTarget(dev(X, engine), dev(y, engine), dev(Z, engine), engine=engine)
    cpu = ggp_amd.SgpmcTarget(T(X), T(y), T(Z), engine=SgpmcOracleEngine())
    kw = dict(seed=13, start=cpu.start(), num_adaptation_steps=10)
    a, b = ggp_amd.sample_hmc(gpu, 20, 0, **kw), ggp_amd.sample_hmc(cpu, 20, 0, **kw)
    assert np.array_equal(a.get_sampler_stats("is_accepted"), b.get_sampler_stats("is_accepted"))
    assert np.array_equal(a.get_sampler_stats("step_size"), b.get_sampler_stats("step_size"))
    qa, qb = a["theta_unc"], b["theta_unc"]
    assert np.abs(qa - qb).max() <= 1e-6 * max(1.0, np.abs(qb).max()), np.abs(qa - qb).max()
    assert a.get_sampler_stats("is_accepted").any()


@pytest.mark.gpu
def test_predict_sgpmc_on_the_device_against_the_double(engine):
    X, y, Z = sampler_problem()
    Xs = np.linspace(-3.2, 3.2, 33)[:, None]
    rng = np.random.default_rng(4)
    rows = [{"variance": 0.8 + 0.1 * i, "lengthscales": np.array([0.7 + 0.05 * i]), "noise_variance": 0.05 + 0.01 * i,
             "V": rng.standard_normal(6)} for i in range(3)]
    trace = ggp_amd.Trace(rows, {}, varnames=("variance", "lengthscales", "noise_variance", "V"))
    out = []
    for tgt in (ggp_amd.SgpmcTarget(dev(X, engine), dev(y, engine), dev(Z, engine), engine=engine),
                ggp_amd.SgpmcTarget(T(X), T(y), T(Z), engine=SgpmcOracleEngine())):
        out.append(ggp_amd.predict_sgpmc(ggp_amd.SgpmcModel(tgt), trace, Xs))
    for got, want in zip(out[0], out[1]):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-8, np.abs(got - want).max()
