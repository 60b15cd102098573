"""GPU: SGPMC with the multi-class robust-max likelihood -- sgp_sgpmc_mc_rows, sgp_sgpmc_mc_tail and the two existing reverse calls
behind them against the long-double reference tests/sgpmc_mc_reference.py; ``SgpmcTarget(likelihood="multiclass")`` on the device
against the CPU double.

Every (N, M, d, C) cell is the smallest shape that reaches its branch:

    (1, 1, 1, 2)       the smallest shape                         (300, 129, 9, 5)   Mp = 256 with padded rows; d > 8
    (63, 5, 1, 3)      N < 64, and the ill-conditioned cell        (200, 130, 32, 3)  SGP_MAX_DIM
                       (lengthscale 3.5 spacings)                  (600, 300, 2, 16)  SGP_MAX_CLASSES; V spans three LDS stages of 128
    (255, 64, 2, 3) (256, 64, 2, 3) (257, 65, 3, 4)                                   columns (Mp = 384)
                       either side of the 256-row and the          (65537, 5, 1, 3)   the second stride of the scaling kernel (4112 groups
                       64-column boundaries                                           of 16 rows over 4096 workgroups); the row pass and the
                                                                                      fold have none below 2^18 rows

The first rows of every cell sit on inducing inputs; the cells' jitter keeps their variance above the floor, and one test of its own
lowers the jitter so that they reach it.  Class C-1 has no datum (C > 2).  rbf runs on all cells, matern32 / matern52 on two; V is 0,
standard normal and 30 x standard normal.  Every cell but those with V = 0 (dv = 0 exactly) and 30 x (most data saturate) is asserted to hold rows with dv > 0 AND rows with dv < 0.  The
comparison is component-wise |got - ref| <= MARGIN * max(e64, FLOOR) * A with A the reference's condition scale, MARGIN = 10, FLOOR =
1e-13 (the rule and the constants of tests/test_svgp_kernel.py), e64 the cell's float64 level measured on the CPU by
``sgpmc_mc_reference.measure_e64`` (tests/test_sgpmc_mc_reference.py recomputes the table below).
"""
import numpy as np
import pytest
import torch

from conftest import dev

import ggp_amd
import sgpmc_mc_reference as R
from sgpmc_mc_double import SgpmcMcOracleEngine

MARGIN = 10
FLOOR = 1e-13
# e64 per (N, M, d, C, kernel, scale of V): sgpmc_mc_reference.measure_e64, one significant digit
E64 = {
    (1, 1, 1, 2, 'rbf', 1.0): 1e-16,
    (63, 5, 1, 3, 'rbf', 0.0): 2e-16,
    (63, 5, 1, 3, 'rbf', 1.0): 2e-12,
    (63, 5, 1, 3, 'rbf', 30.0): 2e-12,
    (63, 5, 1, 3, 'matern32', 1.0): 5e-15,
    (255, 64, 2, 3, 'rbf', 1.0): 1e-15,
    (255, 64, 2, 3, 'rbf', 30.0): 1e-15,
    (256, 64, 2, 3, 'rbf', 1.0): 1e-15,
    (256, 64, 2, 3, 'rbf', 0.0): 3e-16,
    (257, 65, 3, 4, 'rbf', 1.0): 9e-16,
    (257, 65, 3, 4, 'matern52', 1.0): 7e-16,
    (300, 129, 9, 5, 'rbf', 1.0): 8e-16,
    (200, 130, 32, 3, 'rbf', 1.0): 1e-15,
    (600, 300, 2, 16, 'rbf', 1.0): 6e-15,
    (65537, 5, 1, 3, 'rbf', 1.0): 1e-14,
}


def all_cells():
    return [(*cell, k, s) for cell in R.CELLS for k, s in R.COMBOS[cell]]


def tolerance(e64):
    return MARGIN * max(e64, FLOOR)


def check(what, got, ref, A, tol, keys):
    """Prints every figure as a multiple of the tolerance, then asserts."""
    w = {k: v / tol for k, v in R.worst(got, ref, A, keys=keys).items()}
    print("SGPMC_MC %s worst |got - ref| / (tol A) = %.3g  %s" % (what, max(w.values()), {k: "%.2g" % v for k, v in w.items()}))
    assert max(w.values()) <= 1.0, (what, w)


def run_chain(engine, inp, kernel, want_adj, poison=False, want_gz=True):
    """kuu -> kuu_factor -> sgpmc_mc_rows -> sgpmc_mc_tail -> suffstats_bwd_factored -> kuu_bwd through the engine; every output as
    numpy under the reference's keys, and the raw device tensors under "raw"."""
    X, y, Z, V = (dev(inp[k], engine) for k in ("X", "y", "Z", "V"))
    N, (M, d), Cn = X.shape[0], Z.shape, V.shape[0]
    ls, sf2 = [float(t) for t in inp["ls"]], float(inp["sf2"])
    Kuu = engine.kuu(Z, ls, sf2, inp["jitter"], kernel)
    linv, info = engine.kuu_factor(Kuu)
    t = engine.kfu_buffer(N, M)
    t.fill_(float("nan"))
    if poison:
        engine._workspace("sgpmc_mc_rows", engine.lib.sgp_sgpmc_mc_rows_workspace_bytes(N, M, d, Cn)).fill_(255)   # all-ones bytes: NaNs
        engine._workspace("sgpmc_mc", engine.lib.sgp_sgpmc_mc_workspace_bytes(M, Cn)).fill_(255)
    rows = engine.sgpmc_mc_rows(X, y, Z, ls, sf2, V, linv, t, kernel, inp["eps"], want_adjoints=want_adj, want_moments=True)
    res = engine.sgpmc_mc_tail(rows, V, N, linv, with_adjoints=want_adj)
    raw = {"out": rows["out"], "dmu": rows["dmu"], "dv": rows["dv"], "tail": res["out"][:5].clone(), "t": t}
    c = lambda a: a.detach().cpu().numpy()
    to = c(res["out"])
    got = {"out": c(rows["out"]), "dmu": c(rows["dmu"]), "dv": c(rows["dv"]), "mu": c(rows["mu"]), "var": c(rows["var"]), "F": to[0],
           "data": to[1], "prior": to[2], "kappabar": to[4]}
    if want_adj:
        zeros_n, zeros_m = torch.zeros(N, dtype=torch.float64, device=engine.device), torch.zeros(M, dtype=torch.float64, device=engine.device)
        g = engine.suffstats_bwd_factored(X, zeros_n, Z, ls, sf2, linv, dev(-2.0 * np.eye(M), engine), 1.0, zeros_m, 0.0, kernel,
                                          want_gz=want_gz, t_in=t)
        engine.kuu_bwd(Z, ls, sf2, res["Kuubar"], g, kernel, want_gz=want_gz)
        raw.update(G=rows["G"], g=rows["g"], vbar=res["vbar"], bbar=res["bbar"], Kuubar=res["Kuubar"], grads=g)
        gh = c(g)
        got.update(G=c(rows["G"]), g=c(rows["g"]), vbar=c(res["vbar"]), bbar=c(res["bbar"]), Kuubar=c(res["Kuubar"]), g_V=c(res["vbar"]),
                   g_ls=gh[:d], g_sf2=gh[d] + to[4] * N)
        if want_gz:
            got["g_Z"] = gh[d + 1:].reshape(M, d)
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    got["raw"] = raw
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,d,Cn,kernel,vscale", all_cells())
def test_rows_tail_and_gradients_against_the_long_double_reference(engine, N, M, d, Cn, kernel, vscale):
    inp = R.cell_inputs(N, M, d, Cn, vscale)
    ref, A = R.cell_reference(N, M, d, Cn, kernel, vscale)
    if vscale == 1.0 and N > 1:
        assert (ref["dv"] > 0).any() and (ref["dv"] < 0).any()          # both signs of dv are in the cell
    if Cn > 2:
        assert not (inp["y"] == Cn - 1).any()                            # one class has no datum
    tol = tolerance(E64[(N, M, d, Cn, kernel, vscale)])
    got = run_chain(engine, inp, kernel, True)
    if vscale == 0.0:
        assert not got["dv"].any()                                       # ties: dv = 0 exactly
    check("%s" % ((N, M, d, Cn, kernel, vscale),), got, ref, A, tol, R.ALL_KEYS + ("mu", "var"))
    # the folded T the row pass leaves for pass 2, zero in the padding
    Mp = (M + 127) // 128 * 128
    Npad = (N + 255) // 256 * 256
    t = got["raw"]["t"][:Npad * Mp].view(Npad, Mp).cpu().numpy()
    assert not t[N:].any() and not t[:, M:].any()
    check("T_in", {"T_in": t[:N, :M]}, ref, A, tol, ("T_in",))


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [(63, 5, 1, 3), (257, 65, 3, 4), (600, 300, 2, 16)])
def test_same_bits_whatever_the_workspace_held_and_value_only_equals_adjoint_F(engine, cell):
    inp = R.cell_inputs(*cell, 1.0)
    a = run_chain(engine, inp, "rbf", True)
    b = run_chain(engine, inp, "rbf", True, poison=True)
    keys = ("out", "dmu", "dv", "tail", "G", "g", "vbar", "bbar", "Kuubar", "grads")
    for k in keys:
        assert torch.equal(a["raw"][k], b["raw"][k]), k
    Mp, Npad = (cell[1] + 127) // 128 * 128, (cell[0] + 255) // 256 * 256
    assert torch.equal(a["raw"]["t"][:Npad * Mp], b["raw"]["t"][:Npad * Mp])
    v = run_chain(engine, inp, "rbf", False, poison=True)
    assert torch.equal(v["raw"]["tail"][:3], a["raw"]["tail"][:3]) and torch.equal(v["raw"]["out"], a["raw"]["out"])
    # value-only: T_out is T itself, finite, zero in the padding
    N, M = cell[0], cell[1]
    t = v["raw"]["t"][:Npad * Mp].view(Npad, Mp).cpu().numpy()
    assert np.isfinite(t).all() and not t[N:].any() and not t[:, M:].any()


FLOOR_JITTER = 1e-13   # below the floor 2^-40 sf2 = 1.2e-12: a datum on an inducing input has var ~ the jitter


@pytest.mark.gpu
def test_a_datum_on_an_inducing_input_reaches_the_variance_floor(engine):
    """The cells' jitter 1e-6 keeps var above the floor; with 1e-13 (K_uu of this cell is well conditioned) the first rows, which sit
    on inducing inputs, fall below it: var is raised to the floor and dv = 0 exactly there."""
    N, M, d, Cn = 257, 65, 3, 4
    inp = dict(R.cell_inputs(N, M, d, Cn, 1.0), jitter=FLOOR_JITTER)
    ref, A = R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], "rbf", inp["V"], inp["eps"])
    r64, _ = R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], "rbf", inp["V"], inp["eps"], dtype=np.float64)
    assert ref["floored"][:3].all() and (r64["floored"] == ref["floored"]).all()
    got = run_chain(engine, inp, "rbf", True)
    assert not got["dv"][ref["floored"]].any()
    check("floor", got, ref, A, tolerance(FLOOR_E64), R.ALL_KEYS)


FLOOR_E64 = 9e-16   # measured on the CPU (tests/test_sgpmc_mc_reference.py::test_measured_e64_of_the_floor_cell)


@pytest.mark.gpu
def test_moments_only_call_matches_the_reference(engine):
    N, M, d, Cn = 257, 65, 3, 4
    inp = R.cell_inputs(N, M, d, Cn, 1.0)
    ref, A = R.cell_reference(N, M, d, Cn, "rbf", 1.0)
    X, Z, V = (dev(inp[k], engine) for k in ("X", "Z", "V"))
    ls, sf2 = [float(t) for t in inp["ls"]], float(inp["sf2"])
    linv, info = engine.kuu_factor(engine.kuu(Z, ls, sf2, inp["jitter"], "rbf"))
    rows = engine.sgpmc_mc_rows(X, None, Z, ls, sf2, V, linv, engine.kfu_buffer(N, M), "rbf", inp["eps"])
    assert set(rows) == {"mu", "var"}
    got = {k: rows[k].cpu().numpy() for k in ("mu", "var")}
    check("moments only", got, ref, A, tolerance(E64[(N, M, d, Cn, "rbf", 1.0)]), ("mu", "var"))


@pytest.mark.gpu
def test_a_bad_label_is_nan_and_never_an_address(engine):
    N, M, d, Cn = 63, 5, 1, 3
    inp = dict(R.cell_inputs(N, M, d, Cn, 1.0))
    y = np.array(inp["y"])
    y[3], y[7], y[11], y[13] = 3.0, -1.0, 0.5, 1e300
    inp["y"] = y
    got = run_chain(engine, inp, "rbf", False)
    assert np.isnan(got["F"]) and np.isnan(got["dv"][[3, 7, 11, 13]]).all()
    ok = np.setdiff1d(np.arange(N), [3, 7, 11, 13])
    ref, _ = R.cell_reference(N, M, d, Cn, "rbf", 1.0)
    assert np.isfinite(got["dv"][ok]).all() and np.allclose(got["dv"][ok], ref["dv"][ok].astype(np.float64), rtol=1e-6, atol=1e-12)


@pytest.mark.gpu
def test_refusals_before_any_launch(engine):
    lib = engine.lib
    N, M, d, Cn = 63, 5, 1, 3
    inp = R.cell_inputs(N, M, d, Cn, 1.0)
    X, y, Z, V = (dev(inp[k], engine) for k in ("X", "y", "Z", "V"))
    ls, sf2 = [float(t) for t in inp["ls"]], float(inp["sf2"])
    linv, _ = engine.kuu_factor(engine.kuu(Z, ls, sf2, inp["jitter"], "rbf"))
    t = engine.kfu_buffer(N, M)
    ws = engine._workspace("sgpmc_mc_rows", lib.sgp_sgpmc_mc_rows_workspace_bytes(N, M, d, 16))
    out, dmu, dv, G, g = engine.empty(3), engine.empty(16, N), engine.empty(N), engine.empty(M, M), engine.empty(16, M)
    out.fill_(7.0)
    p = engine._ptr
    inv = engine._inv_ls(ls, d, "rbf")

    def rows(Cc=Cn, eps=1e-3, kid=0, yy=y, adj=0, GG=G, nbytes=None):
        return lib.sgp_sgpmc_mc_rows(p(X), d, p(yy), p(Z), d, inv, sf2, p(V), Cc, eps, N, M, d, kid, p(linv), adj, p(out), p(GG), p(g), p(dmu),
                                     p(dv), None, None, p(t), p(ws), ws.numel() if nbytes is None else nbytes, None)

    ARG, WSP = -1, -3
    assert rows(Cc=1) == ARG and rows(Cc=17) == ARG and rows(eps=0.0) == ARG and rows(eps=1.0) == ARG and rows(eps=float("nan")) == ARG
    assert rows(kid=3) == ARG and rows(adj=1, GG=None) == ARG and rows(adj=1, yy=None) == ARG and rows(yy=None) == ARG   # (no mu / var)
    assert rows(nbytes=64) == WSP
    assert lib.sgp_sgpmc_mc_rows_workspace_bytes(N, M, d, 1) == 0 and lib.sgp_sgpmc_mc_workspace_bytes(M, 17) == 0
    tws = engine._workspace("sgpmc_mc", lib.sgp_sgpmc_mc_workspace_bytes(M, Cn))
    res = engine.empty(5)
    assert lib.sgp_sgpmc_mc_tail(p(out), None, None, p(V), 1, N, M, 0, p(res), None, None, None, None, p(tws), tws.numel(), None) == ARG
    assert lib.sgp_sgpmc_mc_tail(p(out), None, None, p(V), Cn, N, M, 1, p(res), None, None, None, None, p(tws), tws.numel(), None) == ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # nothing was launched
    # the one-column and the SVGP entry points do not take id 4
    v1 = dev(inp["V"][0], engine)
    ws1 = engine._workspace("sgpmc_lik_rows", lib.sgp_sgpmc_lik_rows_workspace_bytes(N, M, d))
    st = lib.sgp_sgpmc_lik_rows(p(X), d, p(y), p(Z), d, inv, sf2, 1.0, p(v1), N, M, d, 0, ggp_amd._lib.SGP_LIK_MULTICLASS_ROBUSTMAX, p(linv), 0,
                                p(out), None, None, p(dmu), p(dv), p(t), p(ws1), ws1.numel(), None)
    assert st == ARG
    with pytest.raises(ggp_amd._lib.SgpStatusError) as ei:
        svgp_with_id(engine, X, y, Z, ls, sf2, ggp_amd._lib.SGP_LIK_MULTICLASS_ROBUSTMAX)
    assert ei.value.status == ARG
    # N = 0 is legal
    e0 = engine.sgpmc_mc_rows(X[:0], y[:0], Z, ls, sf2, V, linv, engine.kfu_buffer(1, M), "rbf", 1e-3, want_adjoints=True)
    assert not e0["out"].cpu().numpy().any() and not e0["G"].cpu().numpy().any() and not e0["g"].cpu().numpy().any()


def svgp_with_id(engine, X, y, Z, ls, sf2, lik_id):
    """sgp_svgp_elbo through the engine with a raw likelihood id (the name table does not know id 4)."""
    from ggp_amd import engine as E
    M = Z.shape[0]
    m, LS = torch.zeros(M, dtype=torch.float64, device=engine.device), torch.eye(M, dtype=torch.float64, device=engine.device)
    saved = E._likelihood_id
    E._likelihood_id = lambda name: lik_id
    try:
        return engine.svgp_elbo(X, y, Z, ls, sf2, 1.0, m, LS, X.shape[0], 1e-6, "rbf", "bernoulli")
    finally:
        E._likelihood_id = saved


@pytest.mark.gpu
def test_target_on_the_device_against_the_cpu_double(engine):
    rng = np.random.default_rng(5)
    N, M, d, Cn = 300, 20, 2, 3
    X = rng.uniform(-2.0, 2.0, (N, d))
    Z = rng.uniform(-2.0, 2.0, (M, d))
    X[:2] = Z[:2]
    y = np.argmax(np.stack([np.sin(2 * X[:, 0]), np.cos(2 * X[:, 1]), 0.3 * X[:, 0] * X[:, 1]], 1) + 0.3 * rng.standard_normal((N, 3)), 1)
    Xt, yt, Zt = torch.as_tensor(X), torch.as_tensor(y.astype(np.float64)), torch.as_tensor(Z)
    t_dev = ggp_amd.SgpmcTarget(Xt.to(engine.device), yt.to(engine.device), Zt.to(engine.device), engine=engine, likelihood="multiclass")
    t_cpu = ggp_amd.SgpmcTarget(Xt, yt, Zt, engine=SgpmcMcOracleEngine(), likelihood="multiclass")
    assert t_dev.ndim == t_cpu.ndim == d + 1 + M * Cn
    for k, vs in enumerate((0.0, 1.0, 3.0)):
        q = np.concatenate([np.asarray(t_cpu.start()[:1 + d]) + 0.3 * rng.standard_normal(1 + d), vs * rng.standard_normal(M * Cn)])
        a, b = t_dev.logp_and_grad(q, want_gz=True), t_cpu.logp_and_grad(q, want_gz=True)
        ga, gb = np.asarray(a[1]), np.asarray(b[1])
        print("SGPMC_MC target %d: logp %.15g vs %.15g, grad err %.3g of %.3g, gz err %.3g" %
              (k, a[0], b[0], np.abs(ga - gb).max(), np.abs(gb).max(), float((a[2].cpu() - b[2]).abs().max())))
        # both sides are float64 evaluations of the same density at a well-conditioned K_uu (jitter 1e-5): 1e-9 relative leaves three
        # orders above the float64 level of the cells above
        assert abs(a[0] - b[0]) <= 1e-9 * (1.0 + abs(b[0]))
        assert np.abs(ga - gb).max() <= 1e-9 * (1.0 + np.abs(gb).max())
        assert float((a[2].cpu() - b[2]).abs().max()) <= 1e-9 * (1.0 + float(b[2].abs().max()))
        assert t_dev.logp(q) == a[0]


# |mean log predictive probability on the device - on the CPU double| of the demo below.  Both run the same seeded recipe in float64,
# but not the same chain: the 40 L-BFGS iterations of the warm-up and the 80 HMC transitions amplify the 1e-12 differences between
# two float64 evaluations of the gradient (the warm-up's final loss already differs in the fourth digit), so the two figures are two
# draws of a 40-sample Monte-Carlo estimate.  MEASURED_DEMO_GAP is what the MI355X showed; the bound is four times that, an eighth
# of the 0.38 between the model's figure and the uniform baseline -- a wrong kernel moves the figure by that order.
DEMO_TOL = 0.05
MEASURED_DEMO_GAP = 0.013   # device -0.7067 vs CPU double -0.7196 on the GPU box (two CPU hosts differ by 0.0035 between themselves)


@pytest.mark.gpu
def test_train_and_predict_on_the_demo_match_the_cpu_double(engine):
    import test_sgpmc_mc as T
    demo = T.demo_module()
    cpu = demo.run(SgpmcMcOracleEngine(), **T.DEMO_KW)
    gpu = demo.run(engine, **T.DEMO_KW)
    gap = abs(gpu["mean_log_pred_prob"] - cpu["mean_log_pred_prob"])
    print("SGPMC_MC demo: device %.12g (accuracy %.4f) vs CPU double %.12g (accuracy %.4f), gap %.3g; warm-up %s vs %s" %
          (gpu["mean_log_pred_prob"], gpu["accuracy"], cpu["mean_log_pred_prob"], cpu["accuracy"], gap, gpu["warmup"], cpu["warmup"]))
    assert gpu["mean_log_pred_prob"] > gpu["baseline_log_uniform"] and gpu["accuracy"] > gpu["baseline_majority_accuracy"]
    assert gap <= DEMO_TOL
