"""CPU: pins the yardstick tests/vfe_reference.py -- central differences of the long-double F against every gradient component, the
float64 run of the same closed form against every bound fixture of tests/golden and against the oracle, the float64 levels
tests/test_small_reference_gpu.py uses as tolerances, the sharpness of the comparison at the cells marked sharp, and every deliberate
defect (``mutate``) failing it."""
import math

import numpy as np
import pytest
import torch

import sgpmc_comp_reference as CR
import vfe_reference as V
from conftest import golden_names, load_golden
from oracle import composite_oracle as CO
from oracle import vfe_oracle as O
from pass2_reference import LD, kuu_bwd_reference

EPS_LD = float(np.finfo(LD).eps)


def _problem(N, M, d, seed):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rs.standard_normal(N)
    Z = X[rs.permutation(N)[:M]].copy()  # rows of X: r = 0 occurs
    return X.astype(LD), y.astype(LD), Z.astype(LD)


def _step(S_F, A):
    """The step that minimises the long-double estimate  h^2 |F'''| / 6 + eps S_F / h  of a central difference's error, with the
    component's condition scale standing in for |F'''| / 6 (inputs and lengthscales are of order one): h = (eps S_F / 2 A)^(1/3)."""
    return LD(min(1e-4, max(1e-8, (EPS_LD * float(S_F) / (2 * max(float(A), 1e-300))) ** (1.0 / 3.0))))


def _fd_check(F_of, x0, ref_g, A_g, S_F, what):
    """Every component of ``x0`` (a long-double array): |central difference - gradient| <= 1e-9 (A + S_F)."""
    x0 = np.array(x0, LD)
    g, A = np.asarray(ref_g, LD).reshape(x0.shape), np.asarray(A_g, LD).reshape(x0.shape)
    for idx in np.ndindex(*x0.shape):
        h = _step(S_F, A[idx])
        xp, xm = x0.copy(), x0.copy()
        xp[idx] += h
        xm[idx] -= h
        fd = (F_of(xp) - F_of(xm)) / (2 * h)
        assert abs(fd - g[idx]) <= 1e-9 * (A[idx] + S_F), (what, idx, float(fd), float(g[idx]), float(A[idx]), float(h))


@pytest.mark.parametrize("kernel,N,M,d", [("rbf", 12, 5, 2), ("matern32", 11, 4, 2), ("matern52", 9, 4, 1)])
def test_stationary_gradients_against_central_differences_in_long_double(kernel, N, M, d):
    """Every component of g_ls, g_sf2, g_s2 and g_Z (Z rows equal to X rows: the Matern kernels at r = 0) and of the NUTS target."""
    X, y, Z = _problem(N, M, d, 7 * N + M)
    ls, sf2, s2, J = np.array([1.0 + 0.1 * j for j in range(d)], LD), LD(1.3), LD(0.07), 1e-6
    ref, A = V.stationary(X, y, Z, ls, sf2, s2, J, kernel)
    S = A["F"]

    def F(**over):
        a = dict(Z=Z, ls=ls, sf2=sf2, s2=s2)
        a.update(over)
        return V.stationary(X, y, a["Z"], a["ls"], a["sf2"], a["s2"], J, kernel, grads=False)[0]["F"]

    _fd_check(lambda v: F(ls=v), ls, ref["g_ls"], A["g_ls"], S, "ls")
    _fd_check(lambda v: F(sf2=v[0]), [sf2], [ref["g_sf2"]], [A["g_sf2"]], S, "sf2")
    _fd_check(lambda v: F(s2=v[0]), [s2], [ref["g_s2"]], [A["g_s2"]], S, "s2")
    _fd_check(lambda v: F(Z=v), Z, ref["g_Z"], A["g_Z"], S, "Z")
    # the K_uu part of the contraction is pass2_reference.kuu_bwd_reference's (an independent restatement, which rounds its inputs
    # to float64 first: 1e-15 of the scale)
    gu, _ = kuu_bwd_reference(Z, ls, sf2, ref["Kbar_uu"], kernel)
    mine, a_mine = V._contract(Z, Z, ls, sf2, ref["Kbar_uu"], kernel, LD, both=True)
    for k in ("ls", "sf2", "Z"):
        assert np.all(np.abs(np.asarray(gu[k]) - np.asarray(mine[k])) <= 1e-15 * np.asarray(a_mine[k])), k
    # mode 1
    th = np.log(np.concatenate([ls, [np.sqrt(sf2), np.sqrt(s2)]])).astype(LD) + LD(0.05)
    rn, An = V.stationary_nuts(X, y, Z, th, J, kernel)
    g = np.concatenate([rn["g_ls"], [rn["g_sf2"], rn["g_s2"]]])
    a = np.concatenate([An["g_ls"], [An["g_sf2"], An["g_s2"]]])
    _fd_check(lambda v: V.stationary_nuts(X, y, Z, v, J, kernel)[0]["F"], th, g, a, An["F"], "theta")


def test_composite_gradients_against_central_differences_in_long_double():
    """Every parameter slot of co2_block() (periodic x expquad + ratquad + expquad + matern32) and the noise, modes 0 and 1."""
    X, y, Z = _problem(14, 5, 1, 3)
    blk = np.asarray(CO.co2_block(n_per=1.1, l_psmooth=0.9, l_pdecay=1.4, n_med=0.8, l_med=1.2, alpha=1.5, n_trend=1.3, l_trend=2.0,
                                  n_noise=0.6, l_noise=0.7, period=1.1), LD)
    s2, J = LD(0.07), 1e-6
    ref, A = V.composite(X, y, Z, blk, s2, J)
    slots = CR.param_slots(np.asarray(blk, np.float64))
    assert all(ref["g_block"][s] == 0 and A["g_block"][s] == 0 for s in range(CR.COMP_LEN) if s not in slots)

    def F_slots(v):
        b = blk.copy()
        b[slots] = v
        return V.composite(X, y, Z, b, s2, J)[0]["F"]

    _fd_check(F_slots, blk[slots], ref["g_block"][slots], A["g_block"][slots], A["F"], "block")
    _fd_check(lambda v: V.composite(X, y, Z, blk, v[0], J)[0]["F"], [s2], [ref["g_s2"]], [A["g_s2"]], A["F"], "s2")
    amps = CR.amp_slots(np.asarray(blk, np.float64))
    free = [(s, 0 if s in amps else (1 if (s - 1) % 8 in (3, 6) else 2), 1.5) for s in slots]
    th = np.log(np.array([np.sqrt(blk[s]) if r == 0 else blk[s] for s, r, _ in free] + [np.sqrt(s2)], LD)) + LD(0.05)
    rn, An = V.composite_nuts(X, y, Z, blk, free, th, J)
    _fd_check(lambda v: V.composite_nuts(X, y, Z, blk, free, v, J)[0]["F"], th, np.concatenate([rn["g_free"], [rn["g_s2"]]]),
              np.concatenate([An["g_free"], [An["g_s2"]]]), An["F"], "theta")


@pytest.mark.parametrize("order", ["inverse", "substitution"])
@pytest.mark.parametrize("name", golden_names())
def test_float64_reference_against_the_golden_fixtures_and_the_oracle(name, order):
    """The closed form in float64 against every bound fixture (from the dense N x N definition) and against the oracle's PyMC3-order
    value and analytic gradients, at the tolerances the fixtures carry (tests/test_oracle_golden.py)."""
    G = load_golden(name)
    sf2, s2, J, kid = float(G["sf2"]), float(G["s2"]), float(G["jitter"]), int(G["kernel_id"])
    r, _ = V.stationary(G["X"], G["y"], G["Z"], G["ls"], sf2, s2, J, kid, np.float64, order)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    Fo = float(O.vfe_pymc3_order(T(G["X"]), T(G["y"]), T(G["Z"]), T(G["ls"]), math.sqrt(sf2), math.sqrt(s2), J, kid))
    go = O.grads_analytic(T(G["X"]), T(G["y"]), T(G["Z"]), T(G["ls"]), sf2, s2, J, kid)
    tol = 1e-9 * max(1.0, abs(float(G["F"])))
    ptol = tol * (1000.0 if float(G["grad_rtol"]) > 1e-6 else 1.0)
    rt, rz = float(G["grad_rtol"]), float(G["gz_rtol"])
    assert abs(r["F"] - float(G["F"])) < tol and abs(r["F"] - Fo) < tol
    assert abs(r["logmarg"] - float(G["logmarg"])) < ptol and abs(r["trace"] - float(G["trace_term"])) < ptol
    for want_ls, want_sf2, want_s2, want_Z in ((G["g_ls"], float(G["g_sf2"]), float(G["g_s2"]), G["g_Z"]),
                                               (go["g_ls"].numpy(), go["g_sf2"], go["g_s2"], go["g_Z"].numpy())):
        assert np.abs(r["g_ls"] - want_ls).max() < rt * max(1.0, np.abs(want_ls).max())
        assert abs(r["g_sf2"] - want_sf2) < rt * max(1.0, abs(want_sf2)) and abs(r["g_s2"] - want_s2) < rt * max(1.0, abs(want_s2))
        assert np.abs(r["g_Z"] - want_Z).max() < rz * max(1.0, np.abs(want_Z).max())


@pytest.mark.parametrize("name", ["co2_d1", "m52_plus_per_rq_d2", "rbf_times_m32_d3"])
def test_float64_composite_reference_against_the_golden_fixtures(name):
    """... and the composite fixtures, at the tolerances tests/test_composite.py holds the device to."""
    import os
    from conftest import GOLDEN_DIR
    G = np.load(os.path.join(GOLDEN_DIR, "composite", name + ".npz"))
    r, _ = V.composite(G["X"], G["y"], G["Z"], G["block"], float(G["s2"]), float(G["jitter"]), np.float64, "substitution")
    sl = CO.grad_slots(G["block"])
    assert abs(r["F"] - float(G["F"])) < 1e-8 * max(1.0, abs(float(G["F"])))
    assert np.abs(r["g_block"][sl] - G["g_block"][sl]).max() < 1e-6 * max(1.0, np.abs(G["g_block"][sl]).max())
    assert abs(r["g_s2"] - float(G["g_s2"])) < 1e-6 * max(1.0, abs(float(G["g_s2"])))


ALL = list(V.CELLS) + [n for n in V.MULTI if n not in V.CELLS]


@pytest.mark.parametrize("name", ALL)
def test_measured_e64_matches_the_table(name):
    """``measure_e64`` recomputes the float64 level of every cell and output group: the table of tests/test_small_reference_gpu.py holds
    it to one significant digit (the rule of tests/test_sgpmc_lik_reference.py; below 1e-16 the figure is the rounding of single
    operations and need not reproduce).  Under the FLOOR of 1e-13 the tolerance does not depend on it at all."""
    import test_small_reference_gpu as G
    e = V.measure_e64(name)
    assert set(G.E64) == set(ALL) and set(G.E64[name]) == set(V.groups_of(name))
    for k, want in G.E64[name].items():
        assert 0.4 * want <= e[k] <= 1.6 * want or max(e[k], want) < 1e-16, (name, k, e[k], want)


@pytest.mark.parametrize("name", list(V.MULTI))
def test_measured_streaming_e64_matches_the_table(name):
    """The same for the streaming order's table (``vfe_reference.streaming64``, the order the device runs, against long double)."""
    import test_small_reference_gpu as G
    e = V.measure_e64_streaming(name)
    assert set(G.E64_STREAM) == set(V.MULTI)
    for k, want in G.E64_STREAM[name].items():
        assert 0.4 * want <= e[k] <= 1.6 * want or max(e[k], want) < 1e-16, (name, k, e[k], want)


SHARP = [n for n, c in V.CELLS.items() if c["sharp"]]
GRAD_BLOCKS = ("g_ls", "g_sf2", "g_s2", "g_Z")


@pytest.mark.parametrize("name", SHARP)
def test_the_comparison_is_sharp_at_the_sharp_cells(name):
    """At the sharp cells the new tolerance lies 100x inside the assertions of tests/test_small.py: tol max(A) <= 1e-8 max|g| for every
    gradient block and tol S_F <= 1e-10 max(1, |F|) -- seeds and lengthscales of the cells were chosen so (rbf with 50 or more
    inducing inputs in one or two dimensions needs a short lengthscale for it)."""
    import test_small_reference_gpu as G
    ref, A = V.cell_reference(name)
    tol = {k: V.tolerance(v) for k, v in G.E64[name].items()}
    assert tol["F"] * float(A["F"]) <= 1e-10 * max(1.0, abs(float(ref["F"])))
    for k in GRAD_BLOCKS:
        assert tol[k] * float(np.max(A[k])) <= 1e-8 * float(np.max(np.abs(ref[k]))), (k, float(np.max(A[k])), float(np.max(np.abs(ref[k]))))


def _applies(mutate, c):
    if mutate in ("matern_h0", "matern_h_nan", "matern_h_rbf"):
        return c["kernel"] != "rbf"
    if mutate == "trace_pad":
        return c["M"] not in (64, 128)
    return True


@pytest.mark.parametrize("mutate", [m for m in V.MUTATIONS if m != "matern_h0"])
def test_every_mutation_fails_at_every_sharp_cell_where_it_applies(mutate):
    """One deliberate defect at a time: at EVERY sharp cell where it applies its worst component exceeds the cell's tolerance (the
    (1, 1, 1) cell has no second row and no pair of distinct points: only the defects in the value's own terms show there)."""
    import test_small_reference_gpu as G
    seen = 0
    for name in SHARP:
        c = V.CELLS[name]
        if not _applies(mutate, c) or (c["N"] == 1 and mutate in ("drop_row", "kuu_z_once", "matern_h_nan", "matern_h_rbf")):
            continue
        ref, A = V.cell_reference(name)
        try:
            bad, _ = V.evaluate(name, mutate=mutate)
        except np.linalg.LinAlgError:  # without the jitter K_uu need not factor at all: that is a failure of the comparison too
            seen += 1
            continue
        w = V.worst(bad, ref, A, V.groups_of(name))
        over = {k: w[k] / V.tolerance(G.E64[name][k]) for k in w}
        print("MUTATION %s at %s: worst / tol = %.3g at %s" % (mutate, name, max(over.values()), max(over, key=over.get)))
        assert max(over.values()) > 1.0, (mutate, name, over)
        seen += 1
    assert seen >= 3, (mutate, seen)


def test_a_zero_matern_slope_at_r_equal_zero_is_no_defect():
    """dk/dr2 at r = 0 set to 0 changes NOTHING: in every term it multiplies d r2 / d theta, which is 0 there (z = x exactly, or the
    diagonal of K_uu) -- so this form cannot be told from the reference and is not among the mutations that must fail.  Two Matern
    defects that can be seen stand in for it: ``matern_h_nan`` (the slope as (dk/dr) / 2r without a guard: 0 / 0 at r = 0, which the
    zero factor does not remove) for the handling of r = 0, and ``matern_h_rbf`` (the rbf's -k/2 for the Matern profile)."""
    for name in ("64-16-2-matern32", "129-48-3-matern52"):
        ref, A = V.cell_reference(name)
        bad, _ = V.evaluate(name, mutate="matern_h0")
        assert max(V.worst(bad, ref, A, V.groups_of(name)).values()) == 0.0
