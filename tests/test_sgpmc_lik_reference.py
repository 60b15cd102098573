"""CPU: pins the yardstick tests/sgpmc_lik_reference.py -- central differences in long double against its own gradients, equality
with tests/sgpmc_reference.py for the Gaussian likelihood (two independent closed forms), the two reuse identities of the device
code, the float64 levels tests/test_sgpmc_lik_gpu.py uses as tolerances, and six deliberate defects standing 100x above them."""
import numpy as np
import pytest

import sgpmc_lik_reference as R
import sgpmc_reference as R0
from pass2_reference import LD

CELL = (63, 5, 1)          # the ill-conditioned cell: small enough for differences in every input
MUT_CELL = (257, 65, 3)    # the mutations are shown on a cell at the tolerance FLOOR


def worst_ratio(got, ref, A):
    """max |got - ref| / A with both sides in long double (``pass2_reference.worst_ratio`` takes ``got`` as a float64 device result)."""
    got, ref, A = (np.asarray(a, LD).reshape(-1) for a in (got, ref, A))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / A)
    return float(np.where(np.isnan(r), LD(np.inf), r).max())


def F_of(inp, kernel, lik, **over):
    a = dict(inp, **over)
    return R.reference(a["X"], a["y"], a["Z"], a["ls"], a["sf2"], a["s2"], a["jitter"], kernel, lik, a["v"], grads=False)[0]["F"]


@pytest.mark.parametrize("kernel,lik", [("rbf", "gaussian"), ("rbf", "bernoulli"), ("matern52", "bernoulli_logit"), ("matern32", "poisson"),
                                        ("rbf", "poisson")])
def test_gradients_against_central_differences_in_long_double(kernel, lik):
    """Every gradient of the reference against (F(x + h) - F(x - h)) / 2h in long double, h = 1e-7 of the input's size: the truncation
    error is h^2 F''' ~ 1e-14 of the gradient's condition scale, the rounding error eps_ld / h ~ 1e-12 of F's; both are inside
    1e-9 (A_gradient + A_F)."""
    inp = {k: (np.asarray(v, LD) if isinstance(v, np.ndarray) else v) for k, v in R.cell_inputs(*CELL, lik, 1.0).items()}
    ref, A = R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["s2"], inp["jitter"], kernel, lik, inp["v"])
    aF = float(A["F"])
    h = LD(1e-7)

    def diff(name, idx=None):
        def at(sign):
            if idx is None:
                return F_of(inp, kernel, lik, **{name: LD(inp[name]) + sign * h})
            x = np.array(inp[name], LD)
            x[idx] += sign * h
            return F_of(inp, kernel, lik, **{name: x})
        return (at(+1) - at(-1)) / (2 * h)

    def close(got, want, a):
        assert abs(got - want) <= 1e-9 * (float(a) + aF), (got, want, float(a))

    for i in range(inp["v"].size):
        close(diff("v", i), ref["g_v"][i], A["g_v"][i])
    close(diff("ls", 0), ref["g_ls"][0], A["g_ls"][0])
    close(diff("sf2"), ref["g_sf2"], A["g_sf2"])
    for m in (0, 3):      # Z[0] is a row of X for the cell's generator or not; both kinds
        close(diff("Z", (m, 0)), ref["g_Z"][m, 0], A["g_Z"][m, 0])
    if lik == "gaussian":
        close(diff("s2"), ref["g_s2"], A["g_s2"])
    else:
        assert ref["g_s2"] == 0


@pytest.mark.parametrize("vscale", [0.0, 1.0, 30.0])
def test_gaussian_equals_the_sgpmc_reference(vscale):
    """Likelihood id 0 against ``sgpmc_reference.reference_at`` -- from the explicit Phi = K_uf K_fu, which amplifies long double's
    own rounding by cond(K_uu): within 1e-17 of that reference's condition scale -- in the value and in the adjoints the two share."""
    inp = R.cell_inputs(*CELL, "gaussian", vscale)
    ref, A = R.cell_reference(*CELL, "rbf", "gaussian", vscale)
    r0, A0 = R0.reference_at(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["s2"], inp["jitter"], 0, inp["v"])
    for k in ("F", "data", "prior", "s2bar", "vbar", "Kuubar"):
        assert worst_ratio(ref[k], r0[k], A0[k]) <= 1e-17, k
    assert worst_ratio(ref["bbar"] / LD(inp["s2"]), r0["bbar"], A0["bbar"]) <= 1e-17
    assert abs(ref["kappabar"] - r0["kappabar"]) <= 1e-18 * abs(r0["kappabar"])
    # ... and in the complete gradient: the Gaussian chain's pass 2 takes Cw = I - v v^T, bbar, kappabar of that reference
    import pass2_reference as P2
    g2, _ = P2.bwd_factored_reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], r0["Linv"], r0["Cw"], inp["s2"], r0["bbar"],
                                      r0["kappabar"], 0)
    gu, _ = P2.kuu_bwd_reference(inp["Z"], inp["ls"], inp["sf2"], r0["Kuubar"], 0)
    for k, mine in (("ls", "g_ls"), ("sf2", "g_sf2"), ("Z", "g_Z")):
        assert worst_ratio(g2[k] + gu[k], ref[mine], A[mine]) <= 1e-15, k


@pytest.mark.parametrize("lik", R._ALL)
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_reuse_identities(kernel, lik):
    """G = -S^T S with S_n = sqrt(-dv_n) a_n^T (dv <= 0), the tail's Kuubar equals the Cholesky adjoint of the row-space route, and the
    factored pass 2's formula under the substitution of include/sgp.h equals the row-space N-side adjoint and gradient."""
    ref, A = R.cell_reference(*MUT_CELL, kernel, lik, 1.0)
    assert (ref["dv"] <= 0).all()
    assert worst_ratio(-(ref["S"].T @ ref["S"]), ref["G"], A["G"]) <= 1e-18
    assert worst_ratio(ref["Kuubar"], ref["row_Kuubar"], A["Kuubar"]) <= 1e-18
    assert worst_ratio(ref["reuse_Kfubar"], ref["row_Kfubar"], A["row_Kfubar"]) <= 1e-18
    for k in R.GRAD_KEYS:
        assert worst_ratio(ref["reuse_" + k], ref[k], A[k]) <= 1e-18, k


SMALL = [(*c, k, l, s) for c in R.CELLS[:5] for k, l, s in R.COMBOS[c]]


@pytest.mark.parametrize("key", SMALL, ids=lambda k: "-".join(str(v) for v in k))
def test_measured_e64_matches_the_table(key):
    """``measure_e64`` recomputes the float64 level of the cells up to (257, 65, 3) (the larger ones, seconds each in long double,
    follow below): the table of tests/test_sgpmc_lik_gpu.py holds it to one significant digit, and no cell reaches the variance floor."""
    import test_sgpmc_lik_gpu as G
    e = R.measure_e64(*key)
    assert 0.4 * G.E64[key] <= e <= 1.6 * G.E64[key] or max(e, G.E64[key]) < 1e-16, (e, G.E64[key])
    assert not R.cell_reference(*key)[0]["floored"].any()
    assert set(G.E64) == {(*c, k, l, s) for c in R.CELLS for k, l, s in R.COMBOS[c]}


LARGE = [(*c, k, l, s) for c in R.CELLS[5:] for k, l, s in R.COMBOS[c]]


@pytest.mark.parametrize("key", LARGE, ids=lambda k: "-".join(str(v) for v in k))
def test_measured_e64_of_the_larger_cells(key):
    """The same for the cells from (300, 129, 9) up (a few seconds each: numpy has no BLAS for long double)."""
    import test_sgpmc_lik_gpu as G
    e = R.measure_e64(*key)
    assert 0.4 * G.E64[key] <= e <= 1.6 * G.E64[key] or max(e, G.E64[key]) < 1e-16, (e, G.E64[key])
    assert not R.cell_reference(*key)[0]["floored"].any()


def test_measured_e64_of_the_svgp_cells():
    """... and for the table of the new likelihood ids through the SVGP bound."""
    import svgp_reference as SR
    import test_sgpmc_lik_gpu as G
    for key, want in G.SVGP_E64.items():
        B, M, d, kernel, lik = key
        inp = G.svgp_inputs(B, M, d, lik)
        ref, A = G.svgp_ref(inp, kernel, lik)
        r64, _ = G.svgp_ref(inp, kernel, lik, dtype=np.float64)
        e = max(SR.worst(r64, ref, A).values())
        assert 0.4 * want <= e <= 1.6 * want or max(e, want) < 1e-16, (key, e, want)


MUTATION_CASES = [("dv_second_derivative", "bernoulli"), ("dv_second_derivative", "bernoulli_logit"), ("no_low", "poisson"),
                  ("no_kappabar", "poisson"), ("drop_row", "bernoulli_logit"), ("unscaled_T", "poisson"), ("no_lgamma", "poisson")]


@pytest.mark.parametrize("mutate,lik", MUTATION_CASES)
def test_every_mutation_stands_100x_above_the_tolerance(mutate, lik):
    """One deliberate defect at a time, through the route the device takes (the "reuse_" gradients beside the entry points' own
    outputs): its worst component is at least 100 tolerances of the cell away from the reference."""
    import test_sgpmc_lik_gpu as G
    key = (*MUT_CELL, "rbf", lik, 1.0)
    tol = G.tolerance(G.E64[key])
    ref, A = R.cell_reference(*key)
    bad, _ = R.cell_reference(*key, mutate=mutate)
    got = {k: bad[k] for k in R.ROWS_KEYS + R.TAIL_KEYS + ("s2bar", "kappabar")}
    got.update({k: bad["reuse_" + k] for k in R.GRAD_KEYS})
    w = R.worst(got, ref, A)
    print("MUTATION %s %s: worst / tol = %.3g at %s" % (mutate, lik, max(w.values()) / tol, max(w, key=w.get)))
    assert max(w.values()) >= 100 * tol, w
