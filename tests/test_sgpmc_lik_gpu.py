"""GPU: SGPMC with a non-conjugate likelihood -- sgp_sgpmc_lik_rows, sgp_sgpmc_lik_tail and the two existing reverse calls behind them
against the long-double reference tests/sgpmc_lik_reference.py; the two new likelihood ids through the SVGP entry points;
``SgpmcTarget(likelihood=...)`` / ``train_sgp_hmc`` / ``predict_sgpmc`` on the device against the CPU double.

Every (N, M, d) cell is the smallest shape that reaches its branch:

    (1, 1, 1)        the smallest shape                          (300, 129, 9)   Mp = 256 with padded rows; d > 8
    (63, 5, 1)       N < 64, and the ill-conditioned cell         (200, 130, 32)  SGP_MAX_DIM
                     (lengthscale 3.5 spacings)                   (600, 300, 2)   Mp = 384
    (255, 64, 2) (256, 64, 2) (257, 65, 3)                        (65537, 5, 1)   asm_sub = 1, and the second stride of the scaling
                     either side of ASM_ROWS and of the 64 boundaries             kernel: 4112 groups of 16 rows over its 4096 workgroups
                                                                                  (the row-moment kernel has no stride: a workgroup
                                                                                  per 256 rows)

Every cell keeps rows of Z equal to rows of X; none reaches the variance floor (asserted) but the one written for it.  rbf runs on all
cells, matern32 / matern52 on two; all four likelihood ids are exercised; v is 0, standard normal and 30 x standard normal
(sgpmc_lik_reference.COMBOS).  The comparison is component-wise |got - ref| <= tolerance(cell) * A with A the reference's condition
scale and

    tolerance = MARGIN * max(e64, FLOOR),   MARGIN = 10, FLOOR = 1e-13      (the rule and the constants of tests/test_svgp_kernel.py)

e64 the cell's float64 level measured on the CPU by ``sgpmc_lik_reference.measure_e64`` (tests/test_sgpmc_lik_reference.py recomputes
the table below and shows that six deliberate defects stand 100x above the tolerance).

Not covered here: tapered SYRK splits and multi-round launches of the contraction -- they need >= 10^5 rows x M >= 512, beyond what a
long-double reference does in seconds.  tools/sgpmc_lik_rates.py runs those shapes and compares against the CPU double on a row subsample.
"""
import math

import numpy as np
import pytest
import torch

from conftest import dev

import ggp_amd
import sgpmc_lik_reference as R
import svgp_reference as SR
from sgpmc_lik_double import SgpmcLikOracleEngine

MARGIN = 10
FLOOR = 1e-13
# e64 per (N, M, d, kernel, likelihood, scale of v): sgpmc_lik_reference.measure_e64, one significant digit
E64 = {
    (1, 1, 1, 'rbf', 'gaussian', 1.0): 2e-16,
    (1, 1, 1, 'rbf', 'bernoulli', 1.0): 8e-17,
    (1, 1, 1, 'rbf', 'bernoulli_logit', 1.0): 8e-17,
    (1, 1, 1, 'rbf', 'poisson', 1.0): 1e-16,
    (63, 5, 1, 'rbf', 'gaussian', 0.0): 2e-16,
    (63, 5, 1, 'rbf', 'gaussian', 1.0): 1e-12,
    (63, 5, 1, 'rbf', 'gaussian', 30.0): 1e-12,
    (63, 5, 1, 'rbf', 'bernoulli', 0.0): 2e-16,
    (63, 5, 1, 'rbf', 'bernoulli', 1.0): 1e-12,
    (63, 5, 1, 'rbf', 'bernoulli', 30.0): 1e-12,
    (63, 5, 1, 'rbf', 'bernoulli_logit', 0.0): 2e-16,
    (63, 5, 1, 'rbf', 'bernoulli_logit', 1.0): 1e-12,
    (63, 5, 1, 'rbf', 'bernoulli_logit', 30.0): 1e-12,
    (63, 5, 1, 'rbf', 'poisson', 0.0): 2e-16,
    (63, 5, 1, 'rbf', 'poisson', 1.0): 1e-12,
    (63, 5, 1, 'rbf', 'poisson', 30.0): 1e-12,
    (63, 5, 1, 'matern32', 'poisson', 1.0): 2e-15,
    (63, 5, 1, 'matern52', 'bernoulli_logit', 1.0): 2e-14,
    (255, 64, 2, 'rbf', 'poisson', 1.0): 9e-16,
    (255, 64, 2, 'rbf', 'bernoulli', 30.0): 1e-13,
    (256, 64, 2, 'rbf', 'bernoulli_logit', 1.0): 8e-16,
    (256, 64, 2, 'rbf', 'gaussian', 0.0): 6e-16,
    (257, 65, 3, 'rbf', 'gaussian', 1.0): 6e-16,
    (257, 65, 3, 'rbf', 'bernoulli', 1.0): 6e-16,
    (257, 65, 3, 'rbf', 'bernoulli_logit', 1.0): 6e-16,
    (257, 65, 3, 'rbf', 'poisson', 1.0): 6e-16,
    (257, 65, 3, 'matern32', 'bernoulli', 1.0): 4e-16,
    (257, 65, 3, 'matern52', 'poisson', 1.0): 6e-16,
    (300, 129, 9, 'rbf', 'poisson', 1.0): 6e-16,
    (300, 129, 9, 'rbf', 'bernoulli_logit', 30.0): 5e-16,
    (200, 130, 32, 'rbf', 'bernoulli', 1.0): 5e-16,
    (200, 130, 32, 'rbf', 'poisson', 0.0): 1e-16,
    (600, 300, 2, 'rbf', 'poisson', 1.0): 3e-15,
    (65537, 5, 1, 'rbf', 'poisson', 1.0): 3e-16,
    (65537, 5, 1, 'rbf', 'bernoulli_logit', 1.0): 3e-16,
}
SVGP_E64 = {   # (B, M, d, kernel, likelihood) through svgp_reference.reference with this file's reference supplying the likelihoods
    (65, 65, 3, 'rbf', 'bernoulli_logit'): 7e-17,
    (65, 65, 3, 'matern52', 'poisson'): 7e-17,
    (300, 129, 9, 'rbf', 'poisson'): 6e-18,
    (300, 129, 9, 'matern52', 'bernoulli_logit'): 2e-17,
}


def all_cells():
    return [(*cell, k, l, s) for cell in R.CELLS for k, l, s in R.COMBOS[cell]]


def tolerance(e64):
    return MARGIN * max(e64, FLOOR)


def check(what, got, ref, A, tol, keys):
    """Prints every figure as a multiple of the tolerance, then asserts."""
    w = {k: v / tol for k, v in R.worst(got, ref, A, keys=keys).items()}
    print("SGPMC_LIK %s worst |got - ref| / (tol A) = %.3g  %s" % (what, max(w.values()), {k: "%.2g" % v for k, v in w.items()}))
    assert max(w.values()) <= 1.0, (what, w)


def run_chain(engine, inp, kernel, lik, want_adj, poison=False, want_gz=True):
    """kuu -> kuu_factor -> sgpmc_lik_rows -> sgpmc_lik_tail -> suffstats_bwd_factored -> kuu_bwd through the engine; every output as
    numpy under the reference's keys, and the raw device tensors under "raw"."""
    X, y, Z, v = (dev(inp[k], engine) for k in ("X", "y", "Z", "v"))
    N, (M, d) = X.shape[0], Z.shape
    ls, sf2, s2 = [float(t) for t in inp["ls"]], float(inp["sf2"]), float(inp["s2"])
    Kuu = engine.kuu(Z, ls, sf2, inp["jitter"], kernel)
    linv, info = engine.kuu_factor(Kuu)
    t = engine.kfu_buffer(N, M)
    t.fill_(float("nan"))
    if poison:
        engine._workspace("sgpmc_lik_rows", engine.lib.sgp_sgpmc_lik_rows_workspace_bytes(N, M, d)).fill_(255)   # all-ones bytes: NaNs
        engine._workspace("sgpmc", engine.lib.sgp_sgpmc_lik_workspace_bytes(M)).fill_(255)
    rows = engine.sgpmc_lik_rows(X, y, Z, ls, sf2, s2, v, linv, t, kernel, lik, want_adjoints=want_adj)
    res = engine.sgpmc_lik_tail(rows, v, N, linv, with_adjoints=want_adj)
    raw = {"out": rows["out"], "dmu": rows["dmu"], "dv": rows["dv"], "tail": res["out"][:5].clone(), "t": t}
    c = lambda a: a.detach().cpu().numpy()
    to = c(res["out"])
    got = {"out": c(rows["out"]), "dmu": c(rows["dmu"]), "dv": c(rows["dv"]), "F": to[0], "data": to[1], "prior": to[2], "s2bar": to[3],
           "kappabar": to[4]}
    if want_adj:
        g = engine.suffstats_bwd_factored(X, rows["dmu"], Z, ls, sf2, linv, dev(-2.0 * np.eye(M), engine), 1.0, res["bbar"], 0.0, kernel,
                                          want_gz=want_gz, t_in=t)
        engine.kuu_bwd(Z, ls, sf2, res["Kuubar"], g, kernel, want_gz=want_gz)
        raw.update(G=rows["G"], g=rows["g"], vbar=res["vbar"], bbar=res["bbar"], Kuubar=res["Kuubar"], grads=g)
        gh = c(g)
        got.update(G=c(rows["G"]), g=c(rows["g"]), vbar=c(res["vbar"]), bbar=c(res["bbar"]), Kuubar=c(res["Kuubar"]), g_v=c(res["vbar"]),
                   g_ls=gh[:d], g_sf2=gh[d] + to[4] * N, g_s2=to[3])
        if want_gz:
            got["g_Z"] = gh[d + 1:].reshape(M, d)
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    got["raw"] = raw
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("key", all_cells(), ids=lambda k: "-".join(str(v) for v in k))
def test_rows_tail_and_gradient_vs_long_double(engine, key):
    """out, G, g, dmu, dv, the tail's F, vbar, bbar, Kuubar and, after the two existing reverse calls, the complete gradient.  The
    value-only call, a NaN-poisoned workspace and a second call return the same bits; the padding of T_out is zero on return."""
    N, M, d, kernel, lik, vs = key
    inp = R.cell_inputs(N, M, d, lik, vs)
    ref, A = R.cell_reference(N, M, d, kernel, lik, vs)
    assert not ref["floored"].any()
    full = run_chain(engine, inp, kernel, lik, True)
    check(str(key), full, ref, A, tolerance(E64[key]), R.ALL_KEYS)
    raw = full["raw"]
    Np, Mp = (N + 255) // 256 * 256, (M + 127) // 128 * 128
    t = raw["t"][: Np * Mp].reshape(Np, Mp)
    assert bool((t[N:] == 0).all()) and bool((t[:, M:] == 0).all()) and bool(torch.isfinite(t).all())
    again = run_chain(engine, inp, kernel, lik, True, poison=True)["raw"]
    for k in ("out", "dmu", "dv", "G", "g", "tail", "vbar", "bbar", "Kuubar", "grads", "t"):
        assert torch.equal(raw[k], again[k]), k
    val = run_chain(engine, inp, kernel, lik, False, poison=True)["raw"]
    for k in ("out", "dmu", "dv", "tail"):
        assert torch.equal(raw[k][:3] if k == "tail" else raw[k], val[k][:3] if k == "tail" else val[k]), k
    tv = val["t"][: Np * Mp].reshape(Np, Mp)
    assert bool((tv[N:] == 0).all()) and bool((tv[:, M:] == 0).all())
    # T_out = diag(dv) T: three roundings above the subnormal range (entries down to 1e-300 occur: k' far from an inducing input)
    assert bool(((raw["dv"][:, None] * tv[:N, :M] - t[:N, :M]).abs() <= 1e-15 * t[:N, :M].abs() + 1e-290).all())


@pytest.mark.gpu
def test_gaussian_through_the_new_chain_matches_the_existing_one(engine):
    """Likelihood id 0 through sgp_sgpmc_lik_rows against the sgp_sgpmc_from_whitened_stats chain on the same inputs: F and every
    gradient within the sum of the two tolerances (each chain's own: the cell's tolerance on the reference's condition scale)."""
    key = (257, 65, 3, "rbf", "gaussian", 1.0)
    N, M, d, kernel, lik, vs = key
    inp = R.cell_inputs(N, M, d, lik, vs)
    ref, A = R.cell_reference(*key)
    new = run_chain(engine, inp, kernel, lik, True)
    X, y, Z, v = (dev(inp[k], engine) for k in ("X", "y", "Z", "v"))
    ls, sf2, s2 = [float(t) for t in inp["ls"]], float(inp["sf2"]), float(inp["s2"])
    linv, info = engine.kuu_factor(engine.kuu(Z, ls, sf2, inp["jitter"], kernel))
    t = engine.kfu_buffer(N, M)
    packed = engine.suffstats_whitened_rows(X, y, Z, ls, sf2, linv, kernel, t_out=t)
    res = engine.sgpmc_tail(packed, v, s2, N, linv, with_adjoints=True)
    g = engine.suffstats_bwd_factored(X, y, Z, ls, sf2, linv, res["Cw"], s2, res["bbar"], -1.0 / (2.0 * s2), kernel, want_gz=True, t_in=t)
    engine.kuu_bwd(Z, ls, sf2, res["Kuubar"], g, kernel, want_gz=True)
    gh, o = g.cpu().numpy(), res["out"].cpu().numpy()
    old = {"F": o[0], "g_v": res["vbar"].cpu().numpy(), "g_ls": gh[:d], "g_sf2": gh[d], "g_s2": o[3], "g_Z": gh[d + 1:].reshape(M, d)}
    assert int(info.item()) == 0
    check("gaussian new vs existing", {k: new[k] for k in old}, old, A, 2 * tolerance(E64[key]), list(old))
    check("gaussian existing vs reference", old, ref, A, tolerance(E64[key]), list(old))


def tail_inputs(lik):
    """The (63, 5, 1) cell with f_u = L v = +45 everywhere and three labels -1 against it: y f < -39.1 at those data, beyond any
    binary64 erfc / past exp(-z)'s comfortable range.  (Poisson: f_u = +720, exp overflows.)"""
    inp = dict(R.cell_inputs(63, 5, 1, lik, 1.0))
    Zs = inp["Z"] / inp["ls"]
    K = inp["sf2"] * np.exp(-SR._sqdist(Zs, Zs) / 2) + inp["jitter"] * np.eye(5)
    inp["v"] = np.linalg.solve(np.linalg.cholesky(K), np.full(5, 720.0 if lik == "poisson" else 45.0))
    if lik != "poisson":
        y = np.ones(63)
        y[[0, 17, 40]] = -1.0
        inp["y"] = y
    return inp


@pytest.mark.gpu
@pytest.mark.parametrize("lik", ["bernoulli", "bernoulli_logit"])
def test_bernoulli_tails_stay_finite(engine, lik):
    inp = tail_inputs(lik)
    args = (inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["s2"], inp["jitter"], "rbf", lik, inp["v"])
    ref, A = R.reference(*args)
    r64, _ = R.reference(*args, dtype=np.float64)
    assert ref["zmin"] < -39.1 and not ref["floored"].any()
    e64 = max(R.worst(r64, ref, A).values())
    got = run_chain(engine, inp, "rbf", lik, True)
    assert all(np.isfinite(np.asarray(got[k], dtype=np.float64)).all() for k in R.ALL_KEYS)
    check("tail %s (e64 %.1e)" % (lik, e64), got, ref, A, tolerance(e64), R.ALL_KEYS)


@pytest.mark.gpu
def test_poisson_overflow_is_a_value_not_a_fault(engine):
    """mu + var / 2 > 709: exp overflows, out[0] is not finite, nothing faults, and ``SgpmcTarget`` turns it into (-inf, zeros)."""
    inp = tail_inputs("poisson")
    ref, _ = R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], 1.0, inp["jitter"], "rbf", "poisson", inp["v"],
                         dtype=np.float64, grads=False)
    assert float((ref["mu"] + ref["var"] / 2).max()) > 709.0
    for adj in (False, True):
        got = run_chain(engine, inp, "rbf", "poisson", adj)
        assert not math.isfinite(float(got["out"][0])) and not math.isfinite(float(got["F"]))
    t = ggp_amd.SgpmcTarget(dev(inp["X"], engine), dev(inp["y"], engine), dev(inp["Z"], engine), jitter=inp["jitter"], engine=engine,
                            likelihood="poisson")
    q = np.array(t.start())
    q[t.n_theta:] = 2000.0
    lp, g = t.logp_and_grad(q)
    assert lp == -math.inf and g == [0.0] * t.ndim and t.logp(q) == -math.inf
    lp, g = t.logp_and_grad(t.start())
    assert math.isfinite(lp) and all(math.isfinite(x) for x in g)


@pytest.mark.gpu
def test_variance_floor(engine):
    """The one cell written for the floor: jitter 0 and data ON inducing inputs, so var_n cancels to rounding there.  Those rows have
    dv = 0 exactly and the density stays finite."""
    inp = dict(R.cell_inputs(63, 5, 1, "poisson", 1.0))
    inp["ls"] = np.array([0.6])          # well conditioned without jitter
    inp["jitter"] = 0.0
    args = (inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], 1.0, 0.0, "rbf", "poisson", inp["v"])
    ref, A = R.reference(*args)
    r64, _ = R.reference(*args, dtype=np.float64)
    assert ref["floored"].sum() == 3 and (r64["floored"] == ref["floored"]).all()
    e64 = max(R.worst(r64, ref, A).values())
    got = run_chain(engine, inp, "rbf", "poisson", True)
    assert (got["dv"][np.asarray(ref["floored"])] == 0.0).all() and (got["dv"][~np.asarray(ref["floored"])] < 0.0).all()
    check("floor (e64 %.1e)" % e64, got, ref, A, tolerance(e64), R.ALL_KEYS)


# ---------------------------------------------------------------------------------------------
# the two new likelihood ids through the SVGP entry points
# ---------------------------------------------------------------------------------------------
def svgp_inputs(B, M, d, lik):
    inp = dict(SR.cell_inputs(B, M, d, "bernoulli" if lik == "bernoulli_logit" else "gaussian"))
    if lik == "poisson":
        X = inp["X"]
        fn = np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, (1 % d)] + 0.3)
        inp["y"] = np.random.default_rng(B + M).poisson(np.exp(fn)).astype(np.float64)
    inp["s2"] = 1.0
    return inp


def svgp_ref(inp, kernel, lik, ls=None, sf2=None, s2=None, dtype=R.LD):
    return R.svgp_reference_lik(inp["X"], inp["y"], inp["Z"], inp["ls"] if ls is None else ls, inp["sf2"] if sf2 is None else sf2,
                                inp["s2"] if s2 is None else s2, inp["m"], inp["LS"], inp["N_total"], inp["jitter"], kernel, R.LIK[lik],
                                dtype=dtype)


def svgp_check(what, res, k, ref, A, tol):
    import test_svgp_kernel as TK
    got = TK.unpack(res, k)
    w = {key: v / tol for key, v in SR.worst(got, ref, A).items()}
    print("SGPMC_LIK svgp %s worst / (tol A) = %.3g" % (what, max(w.values())))
    assert max(w.values()) <= 1.0, (what, w)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(SVGP_E64), ids=lambda k: "-".join(str(v) for v in k))
def test_svgp_elbo_with_the_new_likelihoods(engine, key):
    import test_svgp_kernel as TK
    B, M, d, kernel, lik = key
    inp = svgp_inputs(B, M, d, lik)
    ref, A = svgp_ref(inp, kernel, lik)
    res = TK.single(engine, inp, kernel, lik, True)
    assert int(res["info"].item()) == 0
    svgp_check(str(key), res, None, ref, A, tolerance(SVGP_E64[key]))
    assert torch.equal(TK.single(engine, inp, kernel, lik, False)["out"], res["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,lik", [("rbf", "bernoulli_logit"), ("matern52", "poisson")])
def test_svgp_elbo_batch_with_the_new_likelihoods(engine, kernel, lik):
    import test_svgp_kernel as TK
    cell = (65, 65, 3)
    inp = svgp_inputs(*cell, lik)
    ls, sf2, s2 = SR.theta_samples(inp, 2)
    res = TK.batch(engine, inp, kernel, lik, True, ls, sf2, s2)
    assert res["info"].cpu().tolist() == [0, 0]
    for k in range(2):
        ref, A = svgp_ref(inp, kernel, lik, ls[k], sf2[k], s2[k])
        svgp_check("batch %s %s k=%d" % (kernel, lik, k), res, k, ref, A, tolerance(SVGP_E64[(*cell, kernel, lik)]))


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def e2e_problem(lik, N, M, d=2, seed=4):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, d))
    Z = rng.uniform(-2.0, 2.0, (M, d))
    f = np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, 1])
    y = rng.poisson(np.exp(f)).astype(np.float64) if lik == "poisson" else (f + 0.3 * rng.standard_normal(N) > 0).astype(np.float64)
    return torch.as_tensor(X), torch.as_tensor(y), torch.as_tensor(Z)


@pytest.mark.gpu
@pytest.mark.parametrize("lik", ["bernoulli", "bernoulli_logit", "poisson"])
def test_target_on_the_device_matches_the_cpu_double(engine, lik):
    X, y, Z = e2e_problem(lik, 300, 12)
    td = ggp_amd.SgpmcTarget(X, y, Z, engine=engine, likelihood=lik)
    tc = ggp_amd.SgpmcTarget(X, y, Z, engine=SgpmcLikOracleEngine(), likelihood=lik)
    rng = np.random.default_rng(8)
    for k in range(3):
        q = np.asarray(td.start()) + np.r_[0.3 * rng.standard_normal(td.n_theta), (0.0, 1.0, 2.0)[k] * rng.standard_normal(td.M)]
        a, b = td.logp_and_grad(q, want_gz=True), tc.logp_and_grad(q, want_gz=True)
        assert abs(a[0] - b[0]) <= 1e-9 * (1.0 + abs(b[0]))
        assert np.allclose(a[1], b[1], rtol=1e-7, atol=1e-8 * (1.0 + np.abs(b[1]).max()))
        assert np.allclose(a[2].cpu().numpy(), b[2].numpy(), rtol=1e-6, atol=1e-8 * (1.0 + float(b[2].abs().max())))
        assert abs(td.logp(q) - a[0]) <= 1e-12 * (1.0 + abs(a[0]))


@pytest.mark.gpu
def test_train_and_predict_poisson(engine):
    X, y, Z = e2e_problem("poisson", 200, 8)
    model, trace, secs = ggp_amd.train_sgp_hmc((X, y), Z, 2, tune=20, num_samples=20, engine=engine, seed=3, likelihood="poisson")
    assert model.likelihood == "poisson" and len(trace) == 20
    assert all(np.isfinite(row["theta_unc"]).all() and np.isfinite(row["V"]).all() for row in trace)
    rate = float(np.mean(trace.get_sampler_stats("is_accepted")))
    assert 0.0 < rate <= 1.0
    pm, ym, ys = ggp_amd.predict_sgpmc(model, trace, X[:7])
    assert pm.shape == (7,) and ym.shape == ys.shape == (20, 7) and np.isfinite(ym).all() and (ys > 0).all()
