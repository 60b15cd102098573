"""GPU: SGPMC with a composite kernel, a white-noise term and a linear mean function -- sgp_sgpmc_comp_rows, sgp_sgpmc_lik_tail,
sgp_sgpmc_comp_bwd and sgp_kuu_bwd against the long-double reference tests/sgpmc_comp_reference.py; ``CompositeSgpmcTarget`` /
``sample_hmc`` / ``predict_sgpmc`` on the device against the CPU double tests/sgpmc_comp_double.py.

Every (N, M, d) cell is the smallest shape that reaches its branch:

    (1, 1, 1)        the smallest shape                          (300, 129, 8)   COMP_MAX_DIM, Mp = 256, padded rows, grad_geom's MC = 256
    (63, 5, 1)       N < 64, and the ill-conditioned cell         (600, 200, 1)   the reference's own shape; grad_geom's one-round branch
    (255, 64, 2) (256, 64, 2) (257, 65, 3)                        (65537, 5, 1)   the second COMP_CHUNK_ROWS chunk and the second stride
                     either side of the 256-row workgroup and of                  of the scaling kernel
                     the 64-column boundary; grad_geom's MC 64 -> 128

The structure is ``co2_sgpmc_kernel()``'s (Periodic x Matern52 + RatQuad + ExpQuad + Matern52), lengthscales 0.8 .. 2 grid spacings,
period 7.3 spacings; white = 0.05 with the linear mean on, white = 0 with it off; all four likelihoods on (63, 5, 1) and (257, 65, 3);
v = 0, N(0, 1), 30 N(0, 1) on (63, 5, 1) (sgpmc_comp_reference.COMBOS).  Every cell keeps rows of Z equal to rows of X; none reaches
the variance floor (asserted) but the one written for it.  The comparison is component-wise |got - ref| <= tolerance(cell) * A with A
the reference's condition scale and

    tolerance = MARGIN * max(e64, FLOOR),   MARGIN = 10, FLOOR = 1e-13      (the rule and the constants of tests/test_svgp_kernel.py)

e64 the cell's float64 level measured on the CPU by ``sgpmc_comp_reference.measure_e64`` (tests/test_sgpmc_comp_reference.py recomputes
the table below and shows that seven deliberate defects stand 100x above the tolerance).
"""
import math

import numpy as np
import pytest
import torch

from conftest import dev

import ggp_amd
import sgpmc_comp_reference as R
from sgpmc_comp_double import SgpmcCompOracleEngine

MARGIN = 10
FLOOR = 1e-13
# e64 per (N, M, d, likelihood, scale of v, white + mean on): sgpmc_comp_reference.measure_e64, one significant digit
E64 = {
    (1, 1, 1, 'gaussian', 1.0, True): 4e-16,
    (63, 5, 1, 'gaussian', 1.0, False): 2e-13,
    (63, 5, 1, 'bernoulli', 1.0, False): 2e-13,
    (63, 5, 1, 'bernoulli_logit', 1.0, False): 2e-13,
    (63, 5, 1, 'poisson', 1.0, False): 2e-13,
    (63, 5, 1, 'gaussian', 0.0, False): 4e-16,
    (63, 5, 1, 'gaussian', 30.0, False): 2e-13,
    (255, 64, 2, 'gaussian', 1.0, True): 2e-15,
    (256, 64, 2, 'gaussian', 1.0, False): 2e-15,
    (257, 65, 3, 'gaussian', 1.0, True): 3e-15,
    (257, 65, 3, 'bernoulli', 1.0, True): 3e-15,
    (257, 65, 3, 'bernoulli_logit', 1.0, True): 3e-15,
    (257, 65, 3, 'poisson', 1.0, True): 3e-15,
    (257, 65, 3, 'gaussian', 1.0, False): 3e-15,
    (300, 129, 8, 'gaussian', 1.0, True): 5e-15,
    (600, 200, 1, 'gaussian', 1.0, True): 3e-15,
    (600, 200, 1, 'gaussian', 1.0, False): 3e-15,
    (65537, 5, 1, 'gaussian', 1.0, True): 9e-16,
}
T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def tolerance(e64):
    return MARGIN * max(e64, FLOOR)


def check(what, got, ref, A, tol, keys=R.ALL_KEYS):
    """Prints every figure as a multiple of the tolerance, then asserts."""
    w = {k: v / tol for k, v in R.worst(got, ref, A, keys=keys).items()}
    print("SGPMC_COMP %s worst |got - ref| / (tol A) = %.3g  %s" % (what, max(w.values()), {k: "%.2g" % v for k, v in w.items()}))
    assert max(w.values()) <= 1.0, (what, w)


def run_chain(engine, inp, lik, want_adj, poison=False):
    """kuu -> kuu_factor -> sgpmc_comp_rows -> sgpmc_lik_tail -> sgpmc_comp_bwd -> kuu_bwd through the engine; every output as numpy
    under the reference's keys, and the raw device tensors under "raw"."""
    X, y, Z, v = (dev(inp[k], engine) for k in ("X", "y", "Z", "v"))
    N, (M, d) = X.shape[0], Z.shape
    block, white, s2 = [float(t) for t in inp["block"]], float(inp["white"]), float(inp["s2"])
    mean = None if inp["c"] is None else (X @ dev(inp["c"], engine) + float(inp["c0"])).contiguous()
    linv, info = engine.kuu_factor(engine.kuu(Z, block, 1.0, float(inp["jitter"]) + white, "composite"))
    t = engine.kfu_buffer(N, M)
    t.fill_(float("nan"))
    if poison:
        engine._workspace("sgpmc_comp_rows", engine.lib.sgp_sgpmc_comp_rows_workspace_bytes(N, M, d)).fill_(255)   # all-ones bytes: NaNs
        engine._workspace("sgpmc_comp_bwd", engine.lib.sgp_sgpmc_comp_bwd_workspace_bytes(N, M, d)).fill_(255)
        engine._workspace("sgpmc", engine.lib.sgp_sgpmc_lik_workspace_bytes(M)).fill_(255)
    rows = engine.sgpmc_comp_rows(X, y, Z, block, white, s2, v, linv, t, lik, mean=mean, want_adjoints=want_adj, want_moments=True)
    res = engine.sgpmc_lik_tail(rows, v, N, linv, with_adjoints=want_adj)
    raw = {"out": rows["out"], "dmu": rows["dmu"], "dv": rows["dv"], "mu": rows["mu"], "var": rows["var"], "tail": res["out"][:5].clone(), "t": t}
    c = lambda a: a.detach().cpu().numpy()
    to, ro = c(res["out"]), c(rows["out"])
    got = {"out": ro, "dmu": c(rows["dmu"]), "dv": c(rows["dv"]), "mu": c(rows["mu"]), "var": c(rows["var"]), "F": to[0], "data": to[1],
           "prior": to[2], "s2bar": to[3], "kappabar": to[4]}
    if want_adj:
        g = torch.zeros(ggp_amd._lib.COMP_LEN + 1, dtype=torch.float64, device=engine.device)
        engine.sgpmc_comp_bwd(X, rows["dmu"], Z, block, t, linv, res["bbar"], out=g)
        n_side = g.clone()
        engine.kuu_bwd(Z, block, 1.0, res["Kuubar"], g, "composite")
        Np, Mp = (N + 255) // 256 * 256, (M + 127) // 128 * 128
        raw.update(G=rows["G"], g=rows["g"], vbar=res["vbar"], bbar=res["bbar"], Kuubar=res["Kuubar"], grads=g, n_side=n_side)
        slots, amps = R.param_slots(inp["block"]), R.amp_slots(inp["block"])
        gh, Kb = c(g), c(res["Kuubar"])
        got.update(G=c(rows["G"]), g=c(rows["g"]), vbar=c(res["vbar"]), bbar=c(res["bbar"]), Kuubar=Kb, g_v=c(res["vbar"]),
                   T_out=c(t[: Np * Mp].reshape(Np, Mp)[:N, :M]), bwd_g_blk=c(n_side)[slots],
                   g_block=np.array([gh[s] + (ro[2] if s in amps else 0.0) for s in slots]), g_white=np.trace(Kb) + ro[2], g_s2=ro[1])
        if mean is not None:
            got.update(g_c=c(X.t() @ rows["dmu"]), g_c0=float(c(rows["dmu"].sum())))
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    got["raw"] = raw
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("key", R.all_cells(), ids=lambda k: "-".join(str(v) for v in k))
def test_rows_tail_and_gradient_vs_long_double(engine, key):
    """Every output of sgp_sgpmc_comp_rows, of the tail, of sgp_sgpmc_comp_bwd and, after sgp_kuu_bwd, the complete gradient.  The
    value-only call, a NaN-poisoned workspace and T_out and a second call return the same bits; the padding of T_out is zero."""
    N, M, d, lik, vs, extras = key
    inp = R.cell_inputs(*key)
    ref, A = R.cell_reference(*key)
    assert not ref["floored"].any()
    full = run_chain(engine, inp, lik, True)
    check(str(key), full, ref, A, tolerance(E64[key]))
    raw = full["raw"]
    Np, Mp = (N + 255) // 256 * 256, (M + 127) // 128 * 128
    t = raw["t"][: Np * Mp].reshape(Np, Mp)
    assert bool((t[N:] == 0).all()) and bool((t[:, M:] == 0).all()) and bool(torch.isfinite(t).all())
    again = run_chain(engine, inp, lik, True, poison=True)["raw"]
    for k in ("out", "dmu", "dv", "mu", "var", "G", "g", "tail", "vbar", "bbar", "Kuubar", "grads", "n_side", "t"):
        assert torch.equal(raw[k], again[k]), k
    val = run_chain(engine, inp, lik, False, poison=True)["raw"]
    for k in ("out", "dmu", "dv", "mu", "var", "tail"):
        assert torch.equal(raw[k][:3] if k == "tail" else raw[k], val[k][:3] if k == "tail" else val[k]), k
    tv = val["t"][: Np * Mp].reshape(Np, Mp)
    assert bool((tv[N:] == 0).all()) and bool((tv[:, M:] == 0).all())
    # T_out = diag(dv) T: three roundings above the subnormal range
    assert bool(((raw["dv"][:, None] * tv[:N, :M] - t[:N, :M]).abs() <= 1e-15 * t[:N, :M].abs() + 1e-290).all())


@pytest.mark.gpu
def test_moments_only_call_returns_the_same_moments(engine):
    """y = NULL (prediction): mu and var carry the bits of the full call, out is zero, nothing else is needed."""
    key = (257, 65, 3, "gaussian", 1.0, True)
    inp = R.cell_inputs(*key)
    full = run_chain(engine, inp, "gaussian", False)["raw"]
    X, Z, v = (dev(inp[k], engine) for k in ("X", "Z", "v"))
    block, white = [float(t) for t in inp["block"]], float(inp["white"])
    mean = (X @ dev(inp["c"], engine) + float(inp["c0"])).contiguous()
    linv, _ = engine.kuu_factor(engine.kuu(Z, block, 1.0, float(inp["jitter"]) + white, "composite"))
    r = engine.sgpmc_comp_rows(X, None, Z, block, white, 1.0, v, linv, engine.kfu_buffer(257, 65), "gaussian", mean=mean)
    assert torch.equal(r["mu"], full["mu"]) and torch.equal(r["var"], full["var"]) and bool((r["out"] == 0).all())


@pytest.mark.gpu
def test_variance_floor(engine):
    """The one cell written for the floor: jitter 0, white 0 and data ON inducing inputs, so var_n cancels to rounding there.  Those
    rows have dv = 0 exactly and the density stays finite."""
    inp = dict(R.cell_inputs(63, 5, 1, "poisson", 1.0, False))
    inp.update(block=R.co2_block(), jitter=0.0)          # well conditioned without jitter
    ref, A = R.reference_at(inp, "poisson")
    r64, _ = R.reference_at(inp, "poisson", dtype=np.float64)
    assert ref["floored"].sum() == 3 and (r64["floored"] == ref["floored"]).all()
    e64 = max(R.worst(r64, ref, A).values())
    got = run_chain(engine, inp, "poisson", True)
    assert (got["dv"][np.asarray(ref["floored"])] == 0.0).all() and (got["dv"][~np.asarray(ref["floored"])] < 0.0).all()
    check("floor (e64 %.1e)" % e64, got, ref, A, tolerance(e64))


@pytest.mark.gpu
def test_poisson_overflow_is_a_value_not_a_fault(engine):
    """mu + var / 2 > 709: exp overflows, out[0] is not finite, nothing faults, and the target turns it into (-inf, zeros)."""
    inp = dict(R.cell_inputs(63, 5, 1, "poisson", 1.0, False))
    inp.update(block=R.co2_block(), v=np.full(5, 2000.0))
    ref, _ = R.reference_at(inp, "poisson", dtype=np.float64, grads=False)
    assert float((ref["mu"] + ref["var"] / 2).max()) > 709.0
    for adj in (False, True):
        got = run_chain(engine, inp, "poisson", adj)
        assert not math.isfinite(float(got["out"][0])) and not math.isfinite(float(got["F"]))
    t = ggp_amd.CompositeSgpmcTarget(dev(inp["X"], engine), dev(inp["y"], engine), dev(inp["Z"], engine), ggp_amd.co2_sgpmc_kernel(),
                                     white=1.0, mean="linear", likelihood="poisson", engine=engine)
    q = np.array(t.start())
    q[t.n_theta:] = 2000.0
    lp, g = t.logp_and_grad(q)
    assert lp == -math.inf and g == [0.0] * t.ndim and t.logp(q) == -math.inf
    lp, g = t.logp_and_grad(t.start())
    assert math.isfinite(lp) and all(math.isfinite(x) for x in g)


# ---------------------------------------------------------------------------------------------
# the target, the sampler and the predictive on the device against the CPU double
# ---------------------------------------------------------------------------------------------
def target_problem(N, M, d, seed, lik="gaussian"):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 6.0, (N, d))
    f = np.sin(X.sum(1)) + 0.2 * X[:, 0]
    y = rng.poisson(np.exp(f)).astype(np.float64) if lik == "poisson" else f + 0.1 * rng.standard_normal(N)
    Z = X[rng.choice(N, M, replace=False)] + 0.05 * rng.standard_normal((M, d))
    return X, y, Z


def co2_targets(engine, X, y, Z, lik="gaussian"):
    pri = {k: v for k, v in ggp_amd.CO2_SGPMC_PRIORS.items() if lik == "gaussian" or k != "noise_variance"}
    mk = lambda conv, e: ggp_amd.CompositeSgpmcTarget(conv(X), conv(y), conv(Z), ggp_amd.co2_sgpmc_kernel(), priors=pri, white=1.0,
                                                      mean="linear", likelihood=lik, engine=e)
    return mk(lambda a: dev(a, engine), engine), mk(T, SgpmcCompOracleEngine())


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,d,lik", [(37, 5, 1, "gaussian"), (300, 65, 3, "gaussian"), (600, 200, 1, "gaussian"), (300, 65, 3, "poisson")])
def test_target_on_the_device_against_the_cpu_double(engine, N, M, d, lik):
    X, y, Z = target_problem(N, M, d, N + M, lik)
    gpu, cpu = co2_targets(engine, X, y, Z, lik)
    rng = np.random.default_rng(5)
    q = np.asarray(gpu.start()) + np.concatenate([rng.uniform(-0.3, 0.3, gpu.n_theta), 0.5 * rng.standard_normal(M)])
    lp_ref, g_ref = cpu.logp_and_grad(q)
    g_ref = np.asarray(g_ref)
    lp, g = gpu.logp_and_grad(q)
    print("SGPMC_COMP target %s: |dlogp| = %.2e (bound %.1e), |dgrad| / max|g| = %.2e" %
          ((N, M, d, lik), abs(lp - lp_ref), 1e-8 * N, np.abs(np.asarray(g) - g_ref).max() / np.abs(g_ref).max()))
    assert abs(lp - lp_ref) <= 1e-8 * N, (lp, lp_ref)
    assert np.abs(np.asarray(g) - g_ref).max() <= 1e-6 * np.abs(g_ref).max()
    assert abs(gpu.logp(q) - lp_ref) <= 1e-8 * N


@pytest.mark.gpu
def test_marginal_identity_on_the_device(engine):
    """Gaussian, no mean, white = 0: F(m) + M/2 log 2 pi - 1/2 log det B = ``CollapsedBound(kernel="composite", form="whitened")`` at
    the same block and jitter, with m from a host solve of the device's own W = T^T T and u = T^T y."""
    N, M, d = 300, 65, 3
    X, y, Z = target_problem(N, M, d, 11)
    Xd, yd, Zd = dev(X, engine), dev(y, engine), dev(Z, engine)
    block, s2, jitter = [float(t) for t in R.co2_block()], 0.08, 1e-5
    result = engine.result_buffer()
    linv, _ = engine.kuu_factor(engine.kuu(Zd, block, 1.0, jitter, "composite"), info=result[2])
    t = engine.kfu_buffer(N, M)
    zero = torch.zeros(M, dtype=torch.float64, device=engine.device)
    engine.sgpmc_comp_rows(Xd, yd, Zd, block, 0.0, s2, zero, linv, t, "gaussian")
    Tm = t[: 512 * 128].reshape(512, 128)[:N, :M].cpu()
    W, u = Tm.T @ Tm, Tm.T @ T(y)
    B = torch.eye(M, dtype=torch.float64) + W / s2
    m = (torch.linalg.solve(B, u) / s2).to(engine.device)
    rows = engine.sgpmc_comp_rows(Xd, yd, Zd, block, 0.0, s2, m, linv, t, "gaussian", want_adjoints=True)
    res = engine.sgpmc_lik_tail(rows, m, N, linv, with_adjoints=True, result=result)
    o, info = engine.read_result(res["buf"].cpu())
    assert info == 0
    marg = o[0] + 0.5 * M * math.log(2.0 * math.pi) - 0.5 * float(torch.linalg.slogdet(B)[1])
    F = ggp_amd.CollapsedBound(Xd, yd, kernel="composite", jitter=jitter, engine=engine, form="whitened").value(Zd, block, 1.0, s2)[0]
    assert abs(marg - F) <= 1e-8 * N, (marg, F)
    assert float(res["vbar"].abs().max()) <= 1e-8 * N


def one_term_pair(X, y, Z, e_comp, e_rbf, conv):
    """A one-term expquad ``CompositeSgpmcTarget`` (no white, no mean, Gamma(2, 1) priors, jitter 1e-5) and ``SgpmcTarget(kernel="rbf")``."""
    g21 = ("gamma", 2.0, 1.0)
    kern = ggp_amd.CompositeKernel([(1.0, [ggp_amd.Factor("expquad", 1.0)])])
    a = ggp_amd.CompositeSgpmcTarget(conv(X), conv(y), conv(Z), kern, priors={"variance_0": g21, "lengthscale_0_0": g21, "noise_variance": g21},
                                     jitter=1e-5, engine=e_comp)
    return a, ggp_amd.SgpmcTarget(conv(X), conv(y), conv(Z), kernel="rbf", jitter=1e-5, engine=e_rbf)


@pytest.mark.gpu
def test_one_term_expquad_equals_the_rbf_target_on_the_device(engine):
    """d = 1: q = [variance | lengthscale | noise | V] in both classes; logp to 1e-8 N, the gradient to 1e-6 max|g|."""
    X, y, Z = target_problem(300, 33, 1, 21)
    a, b = one_term_pair(X, y, Z, engine, engine, lambda t: dev(t, engine))
    assert a.ndim == b.ndim == 3 + 33
    rng = np.random.default_rng(6)
    q = np.asarray(b.start()) + np.concatenate([rng.uniform(-0.3, 0.3, 3), 0.5 * rng.standard_normal(33)])
    (la, ga), (lb, gb) = a.logp_and_grad(q), b.logp_and_grad(q)
    assert abs(la - lb) <= 1e-8 * 300, (la, lb)
    assert np.abs(np.asarray(ga) - np.asarray(gb)).max() <= 1e-6 * np.abs(gb).max()


def sampler_problem():
    rng = np.random.default_rng(2)
    X = np.sort(rng.uniform(0.0, 6.0, 60))[:, None]
    y = np.sin(2.0 * np.pi * X[:, 0]) * 0.3 + 0.4 * X[:, 0] + 0.1 * rng.standard_normal(60)
    return X, y, np.linspace(0.5, 5.5, 6)[:, None]


@pytest.mark.gpu
def test_same_seed_same_chain_on_the_device_and_over_the_double(engine):
    """N = 60, M = 6, the CO2 structure with white and the mean: twenty transitions (no burn-in, so that the trace shows all twenty) take
    the same accept decisions and step sizes and agree to 1e-6."""
    X, y, Z = sampler_problem()
    gpu, cpu = co2_targets(engine, X, y, Z)
    kw = dict(seed=13, start=cpu.start(), num_leapfrog_steps=20, step_size=0.005, num_adaptation_steps=20, adaptation_rate=0.05)
    a, b = ggp_amd.sample_hmc(gpu, 20, 0, **kw), ggp_amd.sample_hmc(cpu, 20, 0, **kw)
    assert np.array_equal(a.get_sampler_stats("is_accepted"), b.get_sampler_stats("is_accepted"))
    assert np.array_equal(a.get_sampler_stats("step_size"), b.get_sampler_stats("step_size"))
    qa, qb = a["theta_unc"], b["theta_unc"]
    assert np.abs(qa - qb).max() <= 1e-6 * max(1.0, np.abs(qb).max()), np.abs(qa - qb).max()
    assert a.get_sampler_stats("is_accepted").any()


@pytest.mark.gpu
def test_predict_sgpmc_on_the_device_against_the_double(engine):
    X, y, Z = sampler_problem()
    Xs = np.linspace(-0.2, 6.2, 33)[:, None]
    gpu, cpu = co2_targets(engine, X, y, Z)
    rng = np.random.default_rng(4)
    qs = [np.asarray(cpu.start()) + np.concatenate([rng.uniform(-0.3, 0.3, cpu.n_theta), rng.standard_normal(6)]) for _ in range(3)]
    trace = ggp_amd.Trace([{"theta_unc": q} for q in qs], {}, varnames=())
    got = ggp_amd.predict_sgpmc(ggp_amd.CompositeSgpmcModel(gpu), trace, Xs)
    want = ggp_amd.predict_sgpmc(ggp_amd.CompositeSgpmcModel(cpu), trace, Xs)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-8, np.abs(g - w).max()
