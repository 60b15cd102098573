"""CPU: pins the yardstick tests/sgpmc_mc_reference.py -- central differences in long double against its own gradients, the reuse
identities of the device code (the tail's Kuubar, ONE factored pass 2 on the folded T_in), the float64 levels
tests/test_sgpmc_mc_gpu.py uses as tolerances, the facts about dv the issue states, and seven deliberate defects standing 100x above
the tolerance."""
import numpy as np
import pytest

import sgpmc_mc_reference as R
from pass2_reference import LD

CELL = (63, 5, 1, 3)          # the ill-conditioned cell: small enough for differences in every input
MUT_CELL = (257, 65, 3, 4)    # the mutations are shown on a cell at the tolerance FLOOR


def worst_ratio(got, ref, A):
    got, ref, A = (np.asarray(a, LD).reshape(-1) for a in (got, ref, A))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / A)
    return float(np.where(np.isnan(r), LD(np.inf), r).max())


def F_of(inp, kernel, **over):
    a = dict(inp, **over)
    return R.F_of(a["X"], a["y"], a["Z"], a["ls"], a["sf2"], a["jitter"], kernel, a["V"], a["eps"])


@pytest.mark.parametrize("kernel", ["rbf", "matern32", "matern52"])
def test_gradients_against_central_differences_in_long_double(kernel):
    """Every gradient of the reference against (F(x + h) - F(x - h)) / 2h in long double, h = 1e-7: truncation h^2 F''' ~ 1e-14 of the
    gradient's condition scale, rounding eps_ld / h ~ 1e-12 of F's; both are inside 1e-9 (A_gradient + A_F)."""
    inp = {k: (np.asarray(v, LD) if isinstance(v, np.ndarray) else v) for k, v in R.cell_inputs(*CELL, 1.0).items()}
    ref, A = R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], kernel, inp["V"], inp["eps"])
    assert (ref["dv"] > 0).any() and (ref["dv"] < 0).any()
    aF = float(A["F"])
    h = LD(1e-7)

    def diff(name, idx=None):
        def at(sign):
            if idx is None:
                return F_of(inp, kernel, **{name: LD(inp[name]) + sign * h})
            x = np.array(inp[name], LD)
            x[idx] += sign * h
            return F_of(inp, kernel, **{name: x})
        return (at(+1) - at(-1)) / (2 * h)

    def close(got, want, a):
        assert abs(got - want) <= 1e-9 * (float(a) + aF), (got, want, float(a))

    for c in range(CELL[3]):
        for m in range(CELL[1]):
            close(diff("V", (c, m)), ref["g_V"][c, m], A["g_V"][c, m])
    close(diff("ls", 0), ref["g_ls"][0], A["g_ls"][0])
    close(diff("sf2"), ref["g_sf2"], A["g_sf2"])
    for m in (0, 3):
        close(diff("Z", (m, 0)), ref["g_Z"][m, 0], A["g_Z"][m, 0])


@pytest.mark.parametrize("key", [(63, 5, 1, 3, "rbf", 1.0), (63, 5, 1, 3, "rbf", 30.0), (257, 65, 3, 4, "matern52", 1.0)])
def test_reuse_identities(key):
    """The route of the device code (tail's Kuubar + one folded pass 2) equals the row-space gradient to long-double rounding."""
    ref, A = R.cell_reference(*key)
    assert worst_ratio(ref["Kuubar"], ref["row_Kuubar"], A["row_Kuubar"]) < 1e-15
    assert worst_ratio(ref["reuse_Kfubar"], ref["row_Kfubar"], A["row_Kfubar"]) < 1e-15
    for k in R.GRAD_KEYS:
        assert worst_ratio(ref["reuse_" + k], ref[k], A[k]) < 1e-15, k


def test_dv_has_both_signs_and_ties_give_one_over_C():
    """mu = (1, 0, -1), var = 1: dv = -1.14 for y = 0 and +0.49 for y = 2 (the figures of the issue); V = 0 gives p = 1 / C and dv = 0."""
    MU = np.array([[1.0, 0.0, -1.0]] * 2, LD)
    (ell, dMU, dv, p), _ = R.robustmax(np.array([0.0, 2.0], LD), MU, np.ones(2, LD), np.zeros((2, 3)), np.zeros(2), R.EPS, LD)
    assert abs(float(dv[0]) + 1.14) < 0.005 and abs(float(dv[1]) - 0.49) < 0.005
    assert np.abs(dMU.sum(1)).max() < 1e-17                              # a common shift of the means changes nothing
    ref, _ = R.cell_reference(256, 64, 2, 3, "rbf", 0.0)
    assert not ref["dv"].any() and np.abs(ref["p"] - LD(1) / 3).max() < 1e-6


ALL = [(*c, k, s) for c in R.CELLS for k, s in R.COMBOS[c]]


@pytest.mark.parametrize("key", ALL, ids=lambda k: "-".join(str(v) for v in k))
def test_measured_e64_matches_the_table(key):
    """``measure_e64`` recomputes the float64 level of every cell (the largest take a few seconds in long double): the table of
    tests/test_sgpmc_mc_gpu.py holds it to one significant digit.  Levels below the tolerance FLOOR do not enter any tolerance and are
    held to a factor of 4 (they move with the order of summation of the BLAS at hand)."""
    import test_sgpmc_mc_gpu as G
    e = R.measure_e64(*key)
    want = G.E64[key]
    assert 0.4 * want <= e <= 1.6 * want or (max(e, want) < G.FLOOR and 0.25 * want <= e <= 4 * want) or max(e, want) < 1e-16, (e, want)
    assert set(G.E64) == set(ALL)


def test_measured_e64_of_the_floor_cell():
    import test_sgpmc_mc_gpu as G
    N, M, d, Cn = 257, 65, 3, 4
    inp = dict(R.cell_inputs(N, M, d, Cn, 1.0), jitter=G.FLOOR_JITTER)
    args = (inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["jitter"], "rbf", inp["V"], inp["eps"])
    ref, A = R.reference(*args)
    r64, _ = R.reference(*args, dtype=np.float64)
    assert ref["floored"][:3].all() and not ref["dv"][ref["floored"]].any()
    keys = R.ALL_KEYS + tuple("reuse_" + k for k in R.GRAD_KEYS)
    e = max(R.worst({k: r64[k] for k in keys}, ref, A, keys).values())
    assert 0.25 * G.FLOOR_E64 <= e <= 4 * G.FLOOR_E64 < G.FLOOR, e


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_every_mutation_stands_100x_above_the_tolerance(mutate):
    """One deliberate defect at a time, through the route the device takes (the "reuse_" gradients and T_in beside the entry points'
    own outputs): its worst component is at least 100 tolerances of the cell away from the reference."""
    import test_sgpmc_mc_gpu as G
    key = (*MUT_CELL, "rbf", 1.0)
    tol = G.tolerance(G.E64[key])
    ref, A = R.cell_reference(*key)
    bad, _ = R.cell_reference(*key, mutate=mutate)
    got = {k: bad[k] for k in R.ROWS_KEYS + R.TAIL_KEYS + ("T_in",)}
    got.update({k: bad["reuse_" + k] for k in R.GRAD_KEYS})
    w = R.worst(got, ref, A, keys=R.ALL_KEYS + ("T_in",))
    print("MUTATION %s: worst / tol = %.3g at %s" % (mutate, max(w.values()) / tol, max(w, key=w.get)))
    assert max(w.values()) >= 100 * tol, w
