"""CPU: pins the yardstick tests/svgp_mc_reference.py -- its long-double gradients against central differences of its own long-double
bound, the float64 levels tests/test_svgp_mc_gpu.py uses as tolerances (the float64 run of the closed form and the torch-autograd
restatement tests/svgp_mc_double.py, both against the reference), the conditions the issue puts on the cells' inputs, the per-class
derivative formulas at the issue's figures, and six deliberate defects standing 100x above the tolerance."""
import numpy as np
import pytest
import torch

import svgp_mc_reference as R
import test_svgp_mc_gpu as G
from pass2_reference import LD
from svgp_mc_double import SvgpMcOracleEngine

MUT_CELL = (65, 65, 3, 4)     # the mutations are shown on a well-conditioned cell at the tolerance FLOOR
T = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))  # noqa: E731


@pytest.mark.parametrize("cell,kernel", [((63, 5, 1, 3), "rbf"), ((63, 5, 1, 3), "matern32"), ((63, 5, 1, 3), "matern52"), ((64, 64, 2, 3), "rbf")])
def test_gradients_against_central_differences_in_long_double(cell, kernel):
    """One directional derivative per parameter group of the reference's own bound, rows of X on rows of Z present (k(|t|) is even in
    t: a central difference gives their exact zero).  Step 1e-5: truncation ~1e-10 relative, the float64 log Phi adds 1e-16 / 1e-5; the
    allowance is 1e-7 x sum(A o |direction|) (tests/test_svgp_reference.py's)."""
    inp = R.cell_inputs(*cell)
    ref, A = R.cell_reference(*cell, kernel)
    rng = np.random.default_rng(5)
    h = LD(1e-5)

    def value(**over):
        a = {k: (np.asarray(v, dtype=np.float64).astype(LD) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
        a.update(over)
        return R.F_of(a["X"], a["y"], a["Z"], a["ls"], a["sf2"], a["jitter"], kernel, a["m"], a["LS"], a["N_total"], a["eps"])

    for name, key in [("m", "g_m"), ("LS", "g_LS"), ("Z", "g_Z"), ("ls", "g_ls"), ("sf2", "g_sf2")]:
        base = np.asarray(inp[name], dtype=np.float64).astype(LD)
        u = rng.standard_normal(base.shape).astype(LD)
        if name == "LS":
            u = np.tril(u)
        fd = (value(**{name: base + h * u}) - value(**{name: base - h * u})) / (2 * h)
        an = (np.asarray(ref[key], LD) * u).sum()
        scale = float((np.asarray(A[key], LD) * np.abs(u)).sum())
        assert abs(float(fd - an)) <= 1e-7 * scale, (name, float(fd), float(an), scale)
        # ... and in plain terms (the scale of the ill-conditioned cell is 1e9 times its gradients): the step's truncation and the
        # float64 log Phi over the step, 1e-16 |F| / 1e-5, leave 1e-6 of the derivative + 1e-9
        assert abs(float(fd - an)) <= 1e-6 * abs(float(an)) + 1e-9, (name, float(fd), float(an))


def test_per_class_derivatives_at_the_issues_figures():
    """mu = (1, 0, -1), v = 1 for every class: sum_c dv_c is lik_robustmax's gv, -1.137 for y = 0 and +0.486 for y = 2; sum_c dmu_c = 0;
    and with v = 1 the dmu equal sgpmc_mc_reference.robustmax's."""
    import sgpmc_mc_reference as S
    MU, V = np.array([[1.0, 0.0, -1.0]] * 2, LD), np.ones((2, 3), LD)
    y = np.array([0.0, 2.0], LD)
    (ell, dMU, dV, p), _ = R.robustmax_pv(y, MU, V, np.zeros((2, 3)), np.zeros((2, 3)), R.EPS, LD)
    assert abs(float(dV[0].sum()) + 1.137) < 5e-4 and abs(float(dV[1].sum()) - 0.486) < 5e-4
    assert np.abs(dMU.sum(1)).max() < 1e-17
    (ell1, dMU1, dv1, p1), _ = S.robustmax(y, MU, np.ones(2, LD), np.zeros((2, 3)), np.zeros(2), R.EPS, LD)
    assert np.abs(dMU - dMU1).max() < 1e-17 and np.abs(dV.sum(1) - dv1).max() < 1e-17 and np.abs(ell - ell1).max() < 1e-17


def got_of(res):
    return dict(elbo=res["out"][0], ell_sum=res["out"][1], kl=res["out"][2], **{k: res[k] for k in G.GRAD_KEYS})


def double_elbo(inp, kernel):
    return SvgpMcOracleEngine().svgp_mc_elbo(T(inp["X"]), T(inp["y"]), T(inp["Z"]), list(inp["ls"]), inp["sf2"], T(inp["m"]), T(inp["LS"]),
                                             inp["N_total"], inp["eps"], inp["jitter"], kernel, True)


def measure_e64(B, M, d, C, kernel, floor=False):
    """The float64 level of a cell: the worst |float64 - long double| / A over every compared component, of the float64 run of the
    closed form and of the torch-autograd restatement (tests/svgp_mc_double.py)."""
    ref, A = R.cell_reference(B, M, d, C, kernel, floor=floor)
    r64, _ = R.cell_reference(B, M, d, C, kernel, dtype=np.float64, floor=floor)
    dbl = got_of(double_elbo(R.cell_inputs(B, M, d, C, floor), kernel))
    return max(max(R.worst(r64, ref, A).values()), max(R.worst(dbl, ref, A).values()))


def agrees(e, want):
    """One significant digit; levels below the tolerance FLOOR do not enter any tolerance and are held to a factor of 4 (they move with
    the order of summation of the BLAS at hand), those below 1e-16 not at all (tests/test_sgpmc_mc_reference.py's rule)."""
    return 0.4 * want <= e <= 1.6 * want or (max(e, want) < G.FLOOR and 0.25 * want <= e <= 4 * want) or max(e, want) < 1e-16


@pytest.mark.parametrize("key", G.all_cells(), ids=lambda k: "-".join(str(v) for v in k))
def test_measured_e64_matches_the_table(key):
    e = measure_e64(*key)
    print("SVGP_MC e64 %s = %.1e (table %.0e)" % (key, e, G.E64[key]))
    assert agrees(e, G.E64[key]), (e, G.E64[key])
    assert set(G.E64) == set(G.all_cells())


def test_measured_e64_of_the_floor_and_predict_cells():
    e = measure_e64(*R.FLOOR_CELL, "rbf", floor=True)
    assert agrees(e, G.FLOOR_E64) and G.FLOOR_E64 < G.FLOOR, e
    inp = R.cell_inputs(*R.PREDICT_CELL)
    worst = 0.0
    for kernel in ("rbf", "matern52"):
        ref, A = R.predict_cell_reference(kernel, G.PREDICT_T)
        r64, _ = R.predict_cell_reference(kernel, G.PREDICT_T, np.float64)
        mean, var, probs, _ = SvgpMcOracleEngine().svgp_mc_predict(T(inp["X"][:G.PREDICT_T]), T(inp["Z"]), list(inp["ls"]), inp["sf2"],
                                                                   T(inp["m"]), T(inp["LS"]), inp["eps"], inp["jitter"], kernel)
        dbl = {"mean": mean.T, "var": var.T, "probs": probs}
        worst = max(worst, max(R.worst(r64, ref, A, R.PREDICT_KEYS).values()), max(R.worst(dbl, ref, A, R.PREDICT_KEYS).values()))
    assert agrees(worst, G.PREDICT_E64) and G.PREDICT_E64 < G.FLOOR, worst


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_every_mutation_stands_100x_above_the_tolerance(mutate):
    """One deliberate defect at a time: its worst component is at least 100 tolerances of the cell away from the reference (the floor's
    defect on the floor cell, the others on MUT_CELL)."""
    floor = mutate == "floor_dv"
    cell = R.FLOOR_CELL if floor else MUT_CELL
    tol = G.tolerance(G.FLOOR_E64 if floor else G.E64[(*cell, "rbf")])
    ref, A = R.cell_reference(*cell, "rbf", floor=floor)
    bad, _ = R.cell_reference(*cell, "rbf", mutate=mutate, floor=floor)
    w = R.worst(bad, ref, A)
    print("MUTATION %s: worst / tol = %.3g at %s" % (mutate, max(w.values()) / tol, max(w, key=w.get)))
    assert max(w.values()) >= 100 * tol, w


@pytest.mark.parametrize("cell", R.CELLS)
def test_cell_inputs_meet_the_stated_conditions(cell):
    """Conditions on the inputs, asserted on the reference alone (no device value enters)."""
    B, M, d, C = cell
    inp = R.cell_inputs(*cell)
    ref, _ = R.cell_reference(*cell, "rbf", grads=False)
    k = min(3, M, B)
    Zs, Xs = inp["Z"] / inp["ls"], inp["X"] / inp["ls"]
    assert all(bool((Zs == Xs[b]).all(1).any()) for b in range(k))                       # the first rows sit on inducing inputs
    y = inp["y"].astype(np.int64)
    assert ((inp["y"] == y) & (y >= 0) & (y < C)).all()
    if C > 2:
        assert not (y == C - 1).any()                                                    # class C-1 has no datum
    LS = inp["LS"]
    assert all(not np.array_equal(LS[c], LS[0]) for c in range(1, C))                    # the factors differ between the classes
    if M > 1:
        off = LS[:, np.tril_indices(M, -1)[0], np.tril_indices(M, -1)[1]]
        assert (off > 0).any(1).all() and (off < 0).any(1).all()                         # off-diagonal entries of both signs
    assert not ref["floored"].any()                                                      # the cells' jitter keeps v above the floor
    if cell != (1, 1, 1, 2):
        v = np.asarray(ref["v"], np.float64)
        assert (v.max(1) / v.min(1)).max() >= 2.0                                        # per-class variances of one datum differ
        mask = np.ones(v.shape, bool)
        mask[np.arange(B), y] = False
        dv = np.asarray(ref["dv"], np.float64)
        assert (dv[mask] > 0).any() and (dv[mask] < 0).any()                             # dv of the non-labelled classes: both signs
        mu = np.asarray(ref["mu"], np.float64)
        lead = mu[np.arange(B), y] >= mu.max(1)
        assert lead.any() and (~lead).any()                                              # the labelled class leads / trails


def test_the_floor_cell_reaches_the_floor():
    ref, _ = R.cell_reference(*R.FLOOR_CELL, "rbf", floor=True)
    r64, _ = R.cell_reference(*R.FLOOR_CELL, "rbf", dtype=np.float64, floor=True)
    assert ref["floored"][:3, 1].all() and (r64["floored"] == ref["floored"]).all() and not ref["dv"][ref["floored"]].any()
    assert R.cell_inputs(*R.FLOOR_CELL, floor=True)["y"][0] == 1.0
