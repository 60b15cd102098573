"""GPU: the multi-class (robust-max) SVGP bound -- sgp_svgp_mc_elbo and sgp_svgp_mc_predict (csrc/sgp_svgp_mc.hip) against the long-double
reference tests/svgp_mc_reference.py; ``StochasticVariationalGP`` with a ``RobustMaxLikelihood`` on the device against the CPU double.

Every (B, M, d, C) cell is the smallest shape that reaches its branch (the kernels' strides are those of sgp_svgp.hip, the cells the
issue's):

    (1, 1, 1, 2)       the smallest shape                          (300, 129, 9, 5)   Mp = 256 with 127 padded rows; d > 8; the 16-class
    (63, 5, 1, 3)      B < 64, and the ill-conditioned cell                            instantiation of svgp_mc_cols_kernel (C > 4)
                       (lengthscale 3.5 spacings)                  (200, 130, 32, 3)  SGP_MAX_DIM
    (64, 64, 2, 3)     the 64 boundaries (one column block,        (600, 300, 2, 16)  SGP_MAX_CLASSES; Mp = 384, the concatenated product
                       B = Bp)                                                        runs over k = 16 x 384
    (65, 65, 3, 4)     one past them (two column blocks, a         (16385, 5, 1, 3)   the second stride of the likelihood's grid, 256
                       second wave of g_m's rows)                                     workgroups x 64 threads = 16384 data -- the same
    (257, 128, 8, 3)   M = Mp; the 256-lane stride of the                             stride as a 64 x 256 grid
                       contraction kernels

The first rows of every cell sit on inducing inputs (r = 0); class C-1 has no datum (C > 2); the factors LS_c differ between the classes
and have off-diagonal entries of both signs; in every cell but (1, 1, 1, 2) the per-class variances of some datum differ by more than a
factor 2 and dv of the non-labelled classes has both signs (tests/test_svgp_mc_reference.py asserts all of this on the reference).  A cell
of its own (FLOOR_CELL, jitter 1e-13, LS_1 scaled by 1e-25) has variances below the floor 2^-40 sf2.  rbf runs on all cells, matern32 /
matern52 on two.  The comparison is component-wise |got - ref| <= MARGIN * max(e64, FLOOR) * A with A the reference's condition scale,
MARGIN = 10, FLOOR = 1e-13 (the rule and the constants of tests/test_svgp_kernel.py), e64 the cell's float64 level measured on the CPU
(tests/test_svgp_mc_reference.py recomputes the table below).

Rows of probs: the issue asks that they sum to 1 "within the tolerance".  They do not in exact arithmetic: the 20-point rule is not exact
on prod Phi, so sum_c P(c largest) misses 1 by the rule's own error -- 2.3e-5 in the long-double reference at the predict cell, 2.3e-4
at the rows of (65, 65, 3, 4) that sit on inducing inputs (tests/native/lik_mc_host.cpp holds a tie to 1e-3 / C for the same reason).
What is asserted is therefore (a) every entry within the tolerance of the reference, which pins the row sums to the reference's within
tolerance x sum_c A, and (b) the reference's own row sums within 1e-3 of 1, asserted on the reference.
"""
import numpy as np
import pytest
import torch

from conftest import dev

import ggp_amd
import svgp_mc_reference as R

MARGIN = 10
FLOOR = 1e-13
# e64 per (B, M, d, C, kernel): tests/test_svgp_mc_reference.py::measure_e64, one significant digit
E64 = {
    (1, 1, 1, 2, 'rbf'): 5e-17,
    (63, 5, 1, 3, 'rbf'): 3e-17,
    (63, 5, 1, 3, 'matern32'): 3e-17,
    (64, 64, 2, 3, 'rbf'): 4e-17,
    (65, 65, 3, 4, 'rbf'): 3e-17,
    (65, 65, 3, 4, 'matern52'): 3e-17,
    (257, 128, 8, 3, 'rbf'): 4e-18,
    (300, 129, 9, 5, 'rbf'): 2e-16,
    (200, 130, 32, 3, 'rbf'): 2e-17,
    (600, 300, 2, 16, 'rbf'): 1e-16,
    (16385, 5, 1, 3, 'rbf'): 4e-17,
}
FLOOR_E64 = 1e-16     # the floor cell (test_svgp_mc_reference.py::test_measured_e64_of_the_floor_and_predict_cells)
PREDICT_E64 = 4e-16   # mean, var and probs at the predict cell
PREDICT_T = 65        # test rows: two column blocks, the first three on inducing inputs


def all_cells():
    return [(*cell, k) for cell in R.CELLS for k in R.COMBOS[cell]]


def tolerance(e64):
    return MARGIN * max(e64, FLOOR)


def check(what, got, ref, A, tol, keys=R.KEYS):
    """Prints every figure as a multiple of the tolerance, then asserts."""
    w = {k: v / tol for k, v in R.worst(got, ref, A, keys=keys).items()}
    print("SVGP_MC %s worst |got - ref| / (tol A) = %.3g  %s" % (what, max(w.values()), {k: "%.2g" % v for k, v in w.items()}))
    assert max(w.values()) <= 1.0, (what, w)


def run(engine, inp, kernel, with_grads, poison=False, y=None):
    B, (M, d), Cn = inp["X"].shape[0], inp["Z"].shape, inp["m"].shape[0]
    if poison:
        engine._workspace("svgp_mc", engine.lib.sgp_svgp_mc_workspace_bytes(B, M, d, Cn)).fill_(255)   # all-ones bytes: NaNs
    return engine.svgp_mc_elbo(dev(inp["X"], engine), dev(inp["y"] if y is None else y, engine), dev(inp["Z"], engine), list(inp["ls"]),
                               inp["sf2"], dev(inp["m"], engine), dev(inp["LS"], engine), inp["N_total"], eps=inp["eps"],
                               jitter=inp["jitter"], kernel=kernel, with_grads=with_grads)


def unpack(res):
    out = res["out"].cpu()
    got = {"elbo": out[0], "ell_sum": out[1], "kl": out[2]}
    got.update({k: res[k].cpu() for k in ("g_m", "g_LS", "g_Z", "g_ls", "g_sf2") if k in res})
    return got


GRAD_KEYS = ("g_m", "g_LS", "g_Z", "g_ls", "g_sf2")


@pytest.mark.gpu
@pytest.mark.parametrize("key", all_cells(), ids=lambda k: "-".join(str(v) for v in k))
def test_elbo_and_gradients_vs_long_double(engine, key):
    """sgp_svgp_mc_elbo: the bound, sum E log p, KL and the five gradient blocks; the value-only call, a call on a workspace filled with
    all-ones bytes and a second call in a row return the same bits."""
    B, M, d, Cn, kernel = key
    inp = R.cell_inputs(B, M, d, Cn)
    ref, A = R.cell_reference(B, M, d, Cn, kernel)
    res = run(engine, inp, kernel, True)
    assert int(res["info"].item()) == 0 and float(res["out"][3]) == 0.0
    check("elbo %s" % (key,), unpack(res), ref, A, tolerance(E64[key]))
    assert not torch.triu(res["g_LS"], 1).any()
    val = run(engine, inp, kernel, False, poison=True)
    assert torch.equal(val["out"], res["out"])
    again = run(engine, inp, kernel, True, poison=True)
    twice = run(engine, inp, kernel, True)
    for k in ("out",) + GRAD_KEYS:
        assert torch.equal(again[k], res[k]) and torch.equal(twice[k], res[k]), k


@pytest.mark.gpu
def test_variances_below_the_floor(engine):
    """FLOOR_CELL with the jitter lowered to 1e-13 and LS_1 scaled by 1e-25: class 1's variance of the data on inducing inputs is below
    2^-40 sf2 (asserted on the reference); it is raised to the floor and its dv is 0, so every output stays finite and within tolerance."""
    inp = R.cell_inputs(*R.FLOOR_CELL, floor=True)
    ref, A = R.cell_reference(*R.FLOOR_CELL, "rbf", floor=True)
    assert ref["floored"][:3, 1].all() and not ref["dv"][ref["floored"]].any()
    res = run(engine, inp, "rbf", True)
    assert int(res["info"].item()) == 0 and all(bool(torch.isfinite(res[k]).all()) for k in ("out",) + GRAD_KEYS)
    check("floor", unpack(res), ref, A, tolerance(FLOOR_E64))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_predict_vs_long_double(engine, kernel):
    """sgp_svgp_mc_predict at the cell (., 129, 9, 5): latent means, variances and class probabilities at 65 rows (the first three are
    rows of Z); probs = NULL is accepted and changes neither mean nor var."""
    inp = R.cell_inputs(*R.PREDICT_CELL)
    ref, A = R.predict_cell_reference(kernel, PREDICT_T)
    assert np.abs(np.asarray(ref["probs"].sum(1), np.float64) - 1.0).max() <= 1e-3      # the rule's own error, on the reference
    args = (dev(inp["X"][:PREDICT_T], engine), dev(inp["Z"], engine), list(inp["ls"]), inp["sf2"], dev(inp["m"], engine), dev(inp["LS"], engine))
    kw = dict(eps=inp["eps"], jitter=inp["jitter"], kernel=kernel)
    mean, var, probs, info = engine.svgp_mc_predict(*args, **kw)
    assert int(info.item()) == 0 and mean.shape == var.shape == probs.shape == (PREDICT_T, R.PREDICT_CELL[3])
    got = {"mean": mean.cpu().T, "var": var.cpu().T, "probs": probs.cpu()}
    check("predict %s" % kernel, got, ref, A, tolerance(PREDICT_E64), R.PREDICT_KEYS)
    row_tol = tolerance(PREDICT_E64) * A["probs"].sum(1)
    assert (np.abs(probs.cpu().numpy().sum(1) - np.asarray(ref["probs"].sum(1), np.float64)) <= row_tol).all()
    assert (np.abs(probs.cpu().numpy().sum(1) - 1.0) <= 1e-3 + row_tol).all()
    mean2, var2, none, info2 = engine.svgp_mc_predict(*args, want_probs=False, **kw)
    assert none is None and int(info2.item()) == 0 and torch.equal(mean2, mean) and torch.equal(var2, var)


@pytest.mark.gpu
def test_a_bad_label_is_nan_and_never_an_address(engine):
    """Labels 2.5, -1 and C: plain bad data.  out is NaN, the status word stays 0, nothing faults; the gradients of a call with gradients
    are NaN where the bad data reach and the call returns."""
    cell = (63, 5, 1, 3)
    inp = R.cell_inputs(*cell)
    y = np.array(inp["y"])
    y[3], y[7], y[11] = 2.5, -1.0, float(cell[3])
    res = run(engine, inp, "rbf", True, y=y)
    out = res["out"].cpu().numpy()
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.isfinite(out[2]) and out[3] == 0.0 and int(res["info"].item()) == 0
    assert bool(torch.isnan(res["g_m"]).any())


@pytest.mark.gpu
def test_refusals_before_any_launch(engine):
    lib, p = engine.lib, engine._ptr
    B, M, d, Cn = 63, 5, 1, 3
    inp = R.cell_inputs(B, M, d, Cn)
    X, y, Z, m, LS = (dev(inp[k], engine) for k in ("X", "y", "Z", "m", "LS"))
    inv = engine._inv_ls(list(inp["ls"]), d)
    ws = engine._workspace("svgp_mc", lib.sgp_svgp_mc_workspace_bytes(B, M, d, Cn))
    out = engine.empty(4)
    out.fill_(7.0)
    info = torch.zeros(1, dtype=torch.int32, device=engine.device)

    def elbo(Cc=Cn, eps=1e-3, kid=0, grads=0, nbytes=None, dd=d):
        return lib.sgp_svgp_mc_elbo(p(X), dd, p(y), B, p(Z), dd, inv, 1.3, 1e-6, p(m), p(LS), Cc, eps, 10 * B, M, dd, kid, grads, p(out), None, None,
                                    None, None, None, p(info), p(ws), ws.numel() if nbytes is None else nbytes, None)

    ARG, DIM, WSP = -1, -2, -3
    assert elbo(Cc=1) == ARG and elbo(Cc=17) == ARG and elbo(eps=0.0) == ARG and elbo(eps=1.0) == ARG and elbo(eps=float("nan")) == ARG
    assert elbo(kid=3) == ARG and elbo(kid=-1) == ARG and elbo(grads=1) == ARG and elbo(dd=40) == DIM and elbo(nbytes=64) == WSP
    assert lib.sgp_svgp_mc_workspace_bytes(B, M, d, 1) == 0 and lib.sgp_svgp_mc_workspace_bytes(B, M, d, 17) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # nothing was launched


@pytest.mark.gpu
def test_model_on_the_device_against_the_cpu_double(engine):
    """StochasticVariationalGP + RobustMaxLikelihood: one elbo_minibatch and its backward() on the device and on the CPU double (torch
    autograd of the restated forward), at the cell (65, 65, 3, 4) with that cell's m, LS, Z and hyper-parameters; the same tolerance
    rule on the bound and on every parameter's gradient (the raw hyper-parameters' through the softplus chain rule, which both sides
    share: the condition scale of d/dls and d/dsf2 times the softplus derivative)."""
    from svgp_mc_double import SvgpMcOracleEngine
    cell, kernel = (65, 65, 3, 4), "rbf"
    inp = R.cell_inputs(*cell)
    ref, A = R.cell_reference(*cell, kernel)
    tol = tolerance(E64[(*cell, kernel)])

    def build(eng):
        X, y = torch.as_tensor(np.array(inp["X"])), torch.as_tensor(np.array(inp["y"]))
        if eng is engine:
            X, y = X.to(engine.device), y.to(engine.device)
        model = ggp_amd.StochasticVariationalGP(X, y, ggp_amd.RobustMaxLikelihood(cell[3], inp["eps"]), torch.as_tensor(np.array(inp["Z"])),
                                                num_tasks=cell[3], engine=eng, jitter=inp["jitter"])
        model.num_data = inp["N_total"]
        model.covar_module.base_kernel.lengthscale = torch.as_tensor(np.array(inp["ls"]))
        model.covar_module.outputscale = inp["sf2"]
        with torch.no_grad():
            model.variational_mean.copy_(torch.as_tensor(np.array(inp["m"])))
            model.chol_variational_covar.copy_(torch.as_tensor(np.array(inp["LS"])))
        elbo = model.elbo_minibatch(X, y)
        elbo.backward()
        return model, elbo

    md, ed = build(engine)
    mc, ec = build(SvgpMcOracleEngine())
    g = lambda model: {"g_m": model.variational_mean.grad.cpu(), "g_LS": model.chol_variational_covar.grad.cpu(),
                       "g_Z": model.inducing_inputs.grad.cpu()}
    got, want = g(md), g(mc)
    got["elbo"], want["elbo"] = ed.detach().cpu(), ec.detach().cpu()
    check("model vs reference", got, ref, A, tol, ("elbo", "g_m", "g_LS", "g_Z"))
    w = {k: R.worst_ratio(got[k], want[k], A[k]) / tol for k in got}
    # the raw hyper-parameters: d/draw = d/dvalue x softplus'(raw), the factor common to both sides and to the scale
    sl = torch.sigmoid(md.covar_module.base_kernel.raw_lengthscale.detach().cpu()).reshape(-1).numpy()
    so = float(torch.sigmoid(md.covar_module.raw_outputscale.detach().cpu()))
    w["raw_ls"] = R.worst_ratio(md.covar_module.base_kernel.raw_lengthscale.grad.cpu().reshape(-1),
                                mc.covar_module.base_kernel.raw_lengthscale.grad.reshape(-1), A["g_ls"] * sl) / tol
    w["raw_sf2"] = R.worst_ratio(md.covar_module.raw_outputscale.grad.cpu(), mc.covar_module.raw_outputscale.grad, A["g_sf2"] * so) / tol
    print("SVGP_MC model device vs CPU double, multiples of the tolerance: %s" % {k: "%.2g" % v for k, v in w.items()})
    assert max(w.values()) <= 1.0, w    # (the double's own distance from the reference, e64 = 3e-17, is 3e-5 of the tolerance)
