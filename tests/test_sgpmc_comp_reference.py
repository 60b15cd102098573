"""CPU: pins the yardstick tests/sgpmc_comp_reference.py -- central differences in long double against its own gradient, the reuse
identities of the device code against the row-space route, the float64 levels tests/test_sgpmc_comp_gpu.py uses as tolerances, seven
deliberate defects standing 100x above them, and the two conditions on the cells' inputs (no floored row; cond(K_uu) < 1e4 except on
the ill-conditioned cell)."""
import numpy as np
import pytest

import sgpmc_comp_reference as R
from pass2_reference import LD

DIFF_CELL = (63, 5, 1)     # small enough for differences in every input
MUT_CELL = (257, 65, 3)    # the mutations are shown on a cell at the tolerance FLOOR, with white and the mean on


def worst_ratio(got, ref, A):
    """max |got - ref| / A with both sides in long double."""
    got, ref, A = (np.asarray(a, LD).reshape(-1) for a in (got, ref, A))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / A)
    return float(np.where(np.isnan(r), LD(np.inf), r).max())


def diff_inputs(lik):
    """The geometry of DIFF_CELL with the well-conditioned block, white and the mean on: every parameter kind is present."""
    inp = dict(R.cell_inputs(*DIFF_CELL, lik, 1.0, False))
    inp.update(block=R.co2_block(), white=R.WHITE, c=np.full(1, R.MEAN_C), c0=R.MEAN_C0)
    return {k: (np.asarray(v, LD) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


@pytest.mark.parametrize("lik", ["gaussian", "poisson", "bernoulli_logit"])
def test_gradient_against_central_differences_in_long_double(lik):
    """Every entry of the reference's gradient against (F(x + h) - F(x - h)) / 2h in long double, h = 1e-7: truncation h^2 F''' ~ 1e-14
    of the gradient's condition scale, rounding eps_ld / h ~ 1e-12 of F's; both inside 1e-9 (A_gradient + A_F)."""
    inp = diff_inputs(lik)
    ref, A = R.reference_at(inp, lik)
    aF = float(A["F"])
    h = LD(1e-7)

    def diff(name, idx=None):
        def at(sign):
            if idx is None:
                return R.reference_at(dict(inp, **{name: LD(inp[name]) + sign * h}), lik, grads=False)[0]["F"]
            x = np.array(inp[name], LD)
            x[idx] += sign * h
            return R.reference_at(dict(inp, **{name: x}), lik, grads=False)[0]["F"]
        return (at(+1) - at(-1)) / (2 * h)

    def close(got, want, a):
        assert abs(got - want) <= 1e-9 * (float(a) + aF), (got, want, float(a))

    for i in range(inp["v"].size):
        close(diff("v", i), ref["g_v"][i], A["g_v"][i])
    assert ref["slots"] == [1, 4, 5, 7, 9, 12, 13, 17, 20, 25, 28]      # the fixed period's slot 5 included: a block entry like the others
    for k, s in enumerate(ref["slots"]):
        close(diff("block", s), ref["g_block"][k], A["g_block"][k])
    close(diff("white"), ref["g_white"], A["g_white"])
    close(diff("c", 0), ref["g_c"][0], A["g_c"][0])
    close(diff("c0"), ref["g_c0"], A["g_c0"])
    if lik == "gaussian":
        close(diff("s2"), ref["g_s2"], A["g_s2"])
    else:
        assert ref["g_s2"] == 0


@pytest.mark.parametrize("key", [(*MUT_CELL, l, 1.0, True) for l in R._ALL] + [(600, 200, 1, "gaussian", 1.0, False)],
                         ids=lambda k: "-".join(str(v) for v in k))
def test_reuse_identities(key):
    """G = -S^T S (dv <= 0), the tail's Kuubar is the Cholesky adjoint of the row-space route -- its trace and its unsymmetrised
    contraction with dk_uu included --, and -2 T_in L^-1 + dmu w^T is the row-space N-side adjoint."""
    ref, A = R.cell_reference(*key)
    assert (ref["dv"] <= 0).all()
    assert worst_ratio(ref["reuse_G"], ref["G"], A["G"]) <= 1e-18
    assert worst_ratio(ref["Kuubar"], ref["row_Kuubar"], A["Kuubar"]) <= 1e-18
    assert worst_ratio(ref["reuse_Kfubar"], ref["row_Kfubar"], A["row_Kfubar"]) <= 1e-18
    for k in ("bwd_g_blk", "g_block", "g_white"):
        assert worst_ratio(ref["reuse_" + k], ref[k], A[k]) <= 1e-18, k


@pytest.mark.parametrize("key", R.all_cells(), ids=lambda k: "-".join(str(v) for v in k))
def test_measured_e64_matches_the_table_and_the_input_conditions_hold(key):
    """``measure_e64`` recomputes the float64 level of every cell: the table of tests/test_sgpmc_comp_gpu.py holds it to one significant
    digit.  No row of any cell is floored, and cond(K_uu) < 1e4 everywhere but on the ill-conditioned cell, where it is >= 1e4."""
    import test_sgpmc_comp_gpu as G
    e = R.measure_e64(*key)
    assert 0.4 * G.E64[key] <= e <= 1.6 * G.E64[key] or max(e, G.E64[key]) < 1e-16, (e, G.E64[key])
    assert set(G.E64) == set(R.all_cells())
    ref = R.cell_reference(*key)[0]
    assert not ref["floored"].any() and ref["var_over_knn"] > 100 * R.FLOOR_SCALE
    assert (ref["cond"] >= 1e4) if key[:3] == R.ILL_CELL else (ref["cond"] < 1e4), ref["cond"]


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_every_mutation_stands_100x_above_the_tolerance(mutate):
    """One deliberate defect at a time: its worst compared component is at least 100 tolerances of the cell away from the reference."""
    import test_sgpmc_comp_gpu as G
    key = (*MUT_CELL, "poisson", 1.0, True)
    tol = G.tolerance(G.E64[key])
    ref, A = R.cell_reference(*key)
    bad, _ = R.cell_reference(*key, mutate=mutate)
    w = {k: worst_ratio(bad[k], ref[k], A[k]) for k in R.ALL_KEYS}
    print("MUTATION %s: worst / tol = %.3g at %s" % (mutate, max(w.values()) / tol, max(w, key=w.get)))
    assert max(w.values()) >= 100 * tol, w
