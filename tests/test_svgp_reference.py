"""CPU tests that pin tests/svgp_reference.py (the long-double yardstick of the SVGP kernels) and the tolerance tests/test_svgp_kernel.py
allows: against autograd of oracle/svgp_oracle.py, against long-double central differences of the reference's own forward, log Phi against
mpmath, the measured float64 level ``e64`` of every cell (the committed table is recomputed here), and the proof that the comparison
fails on five deliberate defects."""
import numpy as np
import pytest
import torch

import svgp_reference as R
from oracle import svgp_oracle as S
from oracle import vfe_oracle as O
from pass2_reference import LD, worst_ratio
from test_svgp_kernel import E64, FLOOR, MARGIN, all_cells, tolerance

LIKID = {"gaussian": 0, "bernoulli": 1}
ALL = [(k, l) for k in ("rbf", "matern32", "matern52") for l in ("gaussian", "bernoulli")]
T = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))  # noqa: E731


def oracle(inp, kernel, lik):
    return S.svgp_elbo_and_grads(T(inp["X"]), T(inp["y"]), T(inp["Z"]), T(inp["ls"]), inp["sf2"], inp["s2"], T(inp["m"]), T(inp["LS"]),
                                 inp["N_total"], inp["jitter"], R.KID[kernel], LIKID[lik])


def kernel_from_r2_guarded(r2, sf2, kernel_id=0, _plain=O.kernel_from_r2):
    """oracle.vfe_oracle.kernel_from_r2 with the r2 = 0 entries (the diagonal of K_uu, always there) kept away from sqrt: the same
    values, and autograd gives those entries' derivative as 0 -- what an even function of the difference has -- instead of NaN."""
    if kernel_id == 0:
        return _plain(r2, sf2, kernel_id)
    pos = r2 > 0
    return torch.where(pos, _plain(torch.where(pos, r2, torch.ones_like(r2)), sf2, kernel_id), sf2 * torch.ones_like(r2))


@pytest.mark.parametrize("kernel,lik", ALL)
@pytest.mark.parametrize("cell", [(63, 5, 1), (65, 65, 3)])
def test_reference_matches_oracle_autograd(cell, kernel, lik, monkeypatch):
    """X and Z distinct, so that autograd through sqrt(r2) is finite on K_ub for the Matern kernels too (K_uu's own diagonal is
    guarded, see above).  Float64 level: the oracle's own rounding is (chain length ~ M + B) x 1.1e-16 x A at most, 1e-13 A covers
    both cells."""
    monkeypatch.setattr(O, "kernel_from_r2", kernel_from_r2_guarded)
    inp = R.cell_inputs(*cell, lik, distinct=True)
    ref, A = R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["s2"], inp["m"], inp["LS"], inp["N_total"], inp["jitter"],
                         kernel, LIKID[lik])
    w = R.worst(oracle(inp, kernel, lik), ref, A)
    assert set(w) == {"elbo", "g_m", "g_LS", "g_Z", "g_ls", "g_sf2", "g_s2"}
    assert max(w.values()) <= 1e-13, w
    mu, v = S.svgp_predict(T(inp["X"]), T(inp["Z"]), T(inp["ls"]), inp["sf2"], T(inp["m"]), T(inp["LS"]), inp["jitter"], R.KID[kernel])
    (mu_r, v_r), (a_mu, a_v) = R.predict_reference(inp["X"], inp["Z"], inp["ls"], inp["sf2"], inp["m"], inp["LS"], inp["jitter"], kernel)
    assert worst_ratio(mu, mu_r, a_mu) <= 1e-13 and worst_ratio(v, v_r, a_v) <= 1e-13


@pytest.mark.parametrize("kernel,lik", ALL)
@pytest.mark.parametrize("cell", [(63, 5, 1), (64, 64, 2)])
def test_reference_gradients_match_long_double_central_differences(cell, kernel, lik):
    """One directional derivative per parameter group of the reference's own forward, Z subset of X (r = 0 pairs present: k(|t|) is
    even in t, so a central difference gives their exact zero).  Step 1e-5: truncation ~1e-10 relative, the float64 log Phi adds
    1e-16 / 1e-5; the allowance is 1e-7 x sum(A o |direction|)."""
    inp = R.cell_inputs(*cell, lik)
    ref, A = R.cell_reference(*cell, kernel, lik)
    rng = np.random.default_rng(5)
    h = LD(1e-5)

    def value(**over):
        a = {k: (np.asarray(v, dtype=np.float64).astype(LD) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
        a.update(over)
        return R.reference(a["X"], a["y"], a["Z"], a["ls"], a["sf2"], a["s2"], a["m"], a["LS"], a["N_total"], a["jitter"], kernel, LIKID[lik],
                           grads=False)[0]["elbo"]

    groups = [("m", "g_m"), ("LS", "g_LS"), ("Z", "g_Z"), ("ls", "g_ls"), ("sf2", "g_sf2")] + ([("s2", "g_s2")] if lik == "gaussian" else [])
    for name, key in groups:
        base = np.asarray(inp[name], dtype=np.float64).astype(LD)
        u = rng.standard_normal(base.shape).astype(LD)
        if name == "LS":
            u = np.tril(u)
        fd = (value(**{name: base + h * u}) - value(**{name: base - h * u})) / (2 * h)
        an = (np.asarray(ref[key], LD) * u).sum()
        scale = float((np.asarray(A[key], LD) * np.abs(u)).sum())
        assert abs(float(fd - an)) <= 1e-7 * scale, (name, float(fd), float(an), scale)


def test_reference_keeps_long_double_inputs():
    """The central differences above move an input by 1e-5 x u in long double: the reference must not round its inputs to float64."""
    inp = R.cell_inputs(63, 5, 1, "gaussian")
    m = np.asarray(inp["m"]).astype(LD)
    a = [R.reference(inp["X"], inp["y"], inp["Z"], inp["ls"], inp["sf2"], inp["s2"], mm, inp["LS"], inp["N_total"], inp["jitter"], "rbf", 0,
                     grads=False)[0]["elbo"] for mm in (m, m + LD(1e-18))]
    assert a[0] != a[1]


@pytest.mark.parametrize("z", [-45.0, -39.1, -10.0, 0.0, 8.0])
def test_log_ndtr_against_mpmath(z):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    want = mp.log(mp.ncdf(mp.mpf(z)))
    got = float(R.log_ndtr(np.array([z]))[0])
    # two units in the last place where |log Phi| >= log 2; for z > 0, log Phi = log(1 - Phi(-z)) -> -0 and torch's erfc carries
    # ~20 ulp there (4.5e-15 relative at z = 8, on a term of 6e-16): 1e-14, ten times under the floor of the tolerance
    assert abs(got - want) <= (4e-16 if z <= 0 else 1e-14) * abs(want), (z, got, want)
    # phi / Phi as exp(log phi - log Phi), the form the reference takes: the exponent carries |log Phi| x 2.2e-16 (1e-13 at z = -45)
    r = float(np.exp(-LD(z) * LD(z) / 2 - np.log(2 * np.arccos(LD(-1))) / 2 - R.log_ndtr(np.array([z]))[0]))
    want_r = mp.npdf(mp.mpf(z)) / mp.ncdf(mp.mpf(z))
    assert abs(r - want_r) <= 4.4e-16 * max(1.0, abs(float(want))) * want_r, (z, r, want_r)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tolerance is measured
# ---------------------------------------------------------------------------------------------------------------------------------
def measure_e64(cell, kernel, lik, tail=False):
    """Worst component-wise |fp64 - ref| / A of a cell: the fp64 oracle's value (and, under rbf, its autograd gradients -- under a
    Matern kernel they are NaN at the r = 0 pairs every cell holds) and a float64 run of the reference's closed form."""
    inp = R.tail_inputs() if tail else R.cell_inputs(*cell, lik)
    ref, A = R.cell_reference(*cell, kernel, lik, tail=tail)
    o = oracle(inp, kernel, lik)
    if R.KID[kernel] != 0:
        o = {"elbo": o["elbo"]}
    r64, _ = R.cell_reference(*cell, kernel, lik, dtype=np.float64, tail=tail)
    return max(max(R.worst(o, ref, A).values()), max(R.worst(r64, ref, A).values()))


def test_e64_table_is_reproduced():
    """The committed table E64 of tests/test_svgp_kernel.py against a fresh measurement.  What enters the GPU tolerance is
    max(e64, FLOOR): that quantity must agree within 2x for every cell, so the table cannot be tuned to the kernel.  (Every measured
    level is rounding noise of a few 1e-17 .. 1e-15 -- it depends on the BLAS build's summation order --, all below FLOOR = 1e-13; a
    raw figure is additionally held to 20x of the table's, two units in the exponent of noise.)"""
    assert set(E64) == set(all_cells())
    for key in all_cells():
        cell, kernel, lik, tail = key[:3], key[3], key[4], key[-1] == "tail"
        e = measure_e64(cell, kernel, lik, tail)
        eff, tab = max(e, FLOOR), max(E64[key], FLOOR)
        assert tab / 2 <= eff <= 2 * tab, (key, e, E64[key])
        assert E64[key] / 20 <= e <= 20 * E64[key], (key, e, E64[key])


@pytest.mark.parametrize("cell", [(65, 65, 3), (300, 129, 9)])
def test_batch_samples_stay_at_the_cells_level(cell):
    """test_svgp_kernel.py holds every hyper-parameter sample of a batch to its cell's tolerance: the samples' own float64 level stays
    below the floor that tolerance stands on."""
    from test_svgp_kernel import BATCH_COMBOS
    for kernel, lik in BATCH_COMBOS[cell]:
        for k in range(1, 8):
            ref, A = R.cell_reference(*cell, kernel, lik, S=8, k=k)
            r64, _ = R.cell_reference(*cell, kernel, lik, dtype=np.float64, S=8, k=k)
            assert max(R.worst(r64, ref, A).values()) <= FLOOR


def test_cells_are_conditioned_as_stated():
    for cell in R.CELLS:
        inp = R.cell_inputs(*cell, "gaussian")
        Zs = inp["Z"] / inp["ls"]
        c = np.linalg.cond(inp["sf2"] * np.exp(-R._sqdist(Zs, Zs) / 2) + inp["jitter"] * np.eye(cell[1]))
        assert (2e5 <= c <= 2e6) if cell == R.ILL_CELL else c <= 1e4, (cell, c)
        assert bool((Zs[:, None, :] == (inp["X"] / inp["ls"])[None, :, :]).all(-1).any()), cell    # r = 0 is present


# ---------------------------------------------------------------------------------------------------------------------------------
# detection: the comparison fails on deliberate defects
# ---------------------------------------------------------------------------------------------------------------------------------
def exceed(cell, kernel, lik, mutate):
    """By how many tolerances the mutated reference misses the true one on its worst component.  The two mutations of the forward
    are tried on the bound alone first (no reverse pass: the long-double products of the large cell take seconds each)."""
    ref, A = R.cell_reference(*cell, kernel, lik)
    tol = tolerance((*cell, kernel, lik))
    if mutate in ("drop_row", "drop_col"):
        bad, _ = R.cell_reference(*cell, kernel, lik, mutate=mutate, grads=False)
        x = max(R.worst(bad, ref, A, keys=("elbo", "ell_sum")).values()) / tol
        if x >= 100:
            return x
    bad, _ = R.cell_reference(*cell, kernel, lik, mutate=mutate)
    return max(R.worst(bad, ref, A).values()) / tol


DETECT_CELLS = [c for c in R.CELLS if c[1] < 300] + [(1400, 300, 2)]


@pytest.mark.parametrize("cell", DETECT_CELLS)
def test_mutations_are_detected_on_every_cell(cell):
    """Last batch row dropped, last inducing column dropped, Matern-3/2's h used for Matern-5/2: each must stand 100x above the cell's
    tolerance on at least one component, on every cell and every (kernel, likelihood) the GPU test runs there.  The one exception
    is reasoned, not measured: on (1, 1, 1) the only pair has r = 0, where h multiplies a zero difference -- no input of that
    shape with r = 0 present can show a wrong h."""
    for kernel, lik in R.combos(cell):
        for mutate in ("drop_row", "drop_col") + (("h32_for_52",) if kernel == "matern52" and cell != (1, 1, 1) else ()):
            x = exceed(cell, kernel, lik, mutate)
            assert x >= 100, (cell, kernel, lik, mutate, x)


def test_kl_diagonal_term_and_r0_pairs_are_detected():
    """The 1 / diag(L_S) term of the KL gradient omitted; the r = 0 pairs' contribution (to g_sf2: the diagonal of K_uu and the rows
    of X that are rows of Z) omitted.  One cell each is what is asked; every kernel and likelihood on it."""
    for kernel, lik in R.combos((64, 64, 2)):
        assert exceed((64, 64, 2), kernel, lik, "kl_no_invdiag") >= 100
    for kernel, lik in R.combos((16385, 5, 1)):
        assert exceed((16385, 5, 1), kernel, lik, "skip_r0") >= 100
