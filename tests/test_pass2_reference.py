"""The long-double reference of pass 2 (tests/pass2_reference.py) checked on the CPU: against torch autograd and central differences of the
scalar it differentiates, against the oracle engine's float64 restatement, and -- the point of having it -- that the component-wise
comparison |got - ref| <= TAU A NOTICES one missing element.  The comparison functions of tests/test_pass2_kernel.py run here on the
oracle engine, so the GPU tests' own code is exercised without a GPU.

Bounds: float64 autograd and the oracle engine sum at most N M (+ d) products per component, each rounded a handful of times: the
worst case is (chain length) x 2^-53 x A, and what was measured is far below it (2e-16 A for the oracle engine at cells up to
4097 x 257 x 8, 1.5e-14 absolute for autograd at 37 x 5 x 3).  The tests allow 1e-13 A for autograd at N M = 185 terms (worst case 185 x
6 roundings x 1.1e-16 = 1.2e-13) and 1e-14 A for the oracle engine.  Central differences of the long-double scalar at h = 1e-6: truncation
h^2 |f'''| / 6 ~ 1e-12 of the scale, rounding 1e-19 |L| / h ~ 1e-13 |L|: 1e-9 A.
"""
import math

import numpy as np
import pytest
import torch

import pass2_reference as R
import test_pass2_kernel as T
from fake_engine import FactoredOracleEngine, OracleEngine

KERNELS = ("rbf", "matern32", "matern52")


def small(N, M, d, seed, z_rows=False):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone() if z_rows else torch.randn(M, d, dtype=torch.float64, generator=g)
    ls = 0.7 + torch.rand(d, dtype=torch.float64, generator=g) * math.sqrt(d)
    Pb = torch.randn(M, M, dtype=torch.float64, generator=g)          # NOT symmetric
    bb = torch.randn(M, dtype=torch.float64, generator=g)
    return X, y, Z, ls, Pb, bb


def torch_kernel(Xa, Za, ls, sf2, kernel):
    D = (Za[:, None, :] - Xa[None, :, :]) / ls
    r2 = (D * D).sum(-1)
    if kernel == "rbf":
        return sf2 * torch.exp(-0.5 * r2)
    a = torch.sqrt((3.0 if kernel == "matern32" else 5.0) * r2)
    return sf2 * ((1.0 + a) if kernel == "matern32" else (1.0 + a + a * a / 3.0)) * torch.exp(-a)


@pytest.mark.parametrize("kernel", KERNELS)
def test_bwd_reference_against_autograd(kernel):
    N, M, d = 37, 5, 3
    X, y, Z, ls, Pb, bb = small(N, M, d, 3)
    assert float((Pb - Pb.T).abs().max()) > 0.1
    Zt, lst = Z.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    sf2t = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    K = torch_kernel(X, Zt, lst, sf2t, kernel)                          # M x N (random Z: no r = 0, where autograd of sqrt is NaN)
    L = (Pb * (K @ K.T)).sum() + bb @ (K @ y) + (-0.7) * N * sf2t
    L.backward()
    g, A = R.bwd_reference(X, y, Z, ls, 1.7, Pb, bb, -0.7, kernel)
    auto = torch.cat([lst.grad, sf2t.grad.reshape(1), Zt.grad.reshape(-1)])
    R.assert_close(auto, R.pack(g, True), R.pack(A, True), tau=1e-13, what="autograd " + kernel)
    assert abs(float(L.detach()) - float(R.scalar_L(X, y, Z, ls, 1.7, Pb, bb, -0.7, kernel))) < 1e-12 * abs(float(L.detach()))
    # the factored form with Phibar = L^-T (Cw / 2 s2) L^-1 is the same function of an explicit Phibar
    Li = torch.tril(torch.randn(M, M, dtype=torch.float64)) + 2.0 * torch.eye(M, dtype=torch.float64)
    Cw = Pb + Pb.T
    gf, Af = R.bwd_factored_reference(X, y, Z, ls, 1.7, Li, Cw, 0.05, bb, -0.7, kernel)
    ge, Ae = R.bwd_reference(X, y, Z, ls, 1.7, Li.T @ (Cw / 0.1) @ Li, bb, -0.7, kernel)
    R.assert_close(R.pack(ge, True), R.pack(gf, True), R.pack(Af, True), tau=1e-14, what="factored")
    assert bool((R.pack(Af, True) >= R.pack(Ae, True) * (1 - 1e-12)).all())     # |L^-T| |C| |L^-1| >= |L^-T C L^-1|


def central_differences(f, args, h=1e-6):
    """d f / d args[k][i] for every entry of the long-double arrays in ``args`` (f takes them in order)."""
    out = []
    for k, a in enumerate(args):
        gk = np.zeros(a.shape, R.LD)
        for i in np.ndindex(*a.shape):
            up, dn = [v.copy() for v in args], [v.copy() for v in args]
            up[k][i] += R.LD(h)
            dn[k][i] -= R.LD(h)
            gk[i] = (f(*up) - f(*dn)) / (2 * R.LD(h))
        out.append(gk)
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_bwd_reference_at_zero_distance_against_central_differences(kernel):
    """Z = rows of X: r2 = 0 occurs, where dk/dr2 of the Matern profiles is the finite closed form and autograd would give NaN."""
    X, y, Z, ls, Pb, bb = small(23, 4, 2, 5, z_rows=True)
    g, A = R.bwd_reference(X, y, Z, ls, 1.7, Pb, bb, -0.7, kernel)
    f = lambda l, s, z: R.scalar_L(X, y, z, l, s[0], Pb, bb, -0.7, kernel)
    fd = central_differences(f, [R._ld(ls), np.array([1.7], R.LD), R._ld(Z)])
    R.assert_close(np.concatenate([v.reshape(-1) for v in fd]).astype(np.float64), R.pack(g, True), R.pack(A, True), tau=1e-9, what=kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_kuu_bwd_reference_against_central_differences_and_autograd(kernel):
    M, d = 6, 3
    _, _, Z, ls, Kb, _ = small(10, M, d, 8)
    Z[M - 1] = Z[0]                                                    # r2 = 0 off the diagonal too
    g, A = R.kuu_bwd_reference(Z, ls, 1.7, Kb, kernel)                # (a non-symmetric Kuubar: the reference takes any)
    f = lambda l, s, z: R.scalar_Luu(z, l, s[0], Kb, kernel)
    fd = central_differences(f, [R._ld(ls), np.array([1.7], R.LD), R._ld(Z)])
    R.assert_close(np.concatenate([v.reshape(-1) for v in fd]).astype(np.float64), R.pack(g, True), R.pack(A, True), tau=1e-9, what=kernel)
    if kernel == "rbf":                                                # smooth at r = 0: autograd applies
        Zt, lst = Z.clone().requires_grad_(True), ls.clone().requires_grad_(True)
        sf2t = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
        (Kb * torch_kernel(Zt, Zt, lst, sf2t, kernel)).sum().backward()
        auto = torch.cat([lst.grad, sf2t.grad.reshape(1), Zt.grad.reshape(-1)])
        R.assert_close(auto, R.pack(g, True), R.pack(A, True), tau=1e-13, what="autograd")


@pytest.mark.parametrize("N,M,d,kernel", [(1000, 129, 5, "rbf"), (700, 130, 18, "matern52")])
def test_bwd_reference_against_the_oracle_engine(N, M, d, kernel):
    X, y, Z, ls, Pb, bb = small(N, M, d, N + M, z_rows=(kernel != "rbf"))
    g, A = R.bwd_reference(X, y, Z, ls, 1.7, Pb, bb, -0.7, kernel)
    got = OracleEngine().suffstats_bwd(X, y, Z, ls, 1.7, Pb, bb, -0.7, kernel, want_gz=True)
    w = R.assert_close(got, R.pack(g, True), R.pack(A, True), tau=1e-14, what="oracle engine")
    print("oracle engine suffstats_bwd (%d, %d, %d, %s): worst err/A = %.2e" % (N, M, d, kernel, w))
    ratio = (R.pack(A, True) / np.maximum(np.abs(R.pack(g, True)), R.LD(1e-300)))
    assert float(np.median(ratio)) > 5.0                               # random adjoints cancel: why the check is against A, not |g|


@pytest.mark.parametrize("M,d,kernel", [(257, 8, "matern32"), (130, 18, "rbf")])
def test_kuu_bwd_reference_against_the_oracle_engine(M, d, kernel):
    _, _, Z, ls, Kb, _ = small(M, M, d, M + d)
    Kb = Kb + Kb.T
    g, A = R.kuu_bwd_reference(Z, ls, 1.7, Kb, kernel)
    got = OracleEngine().kuu_bwd(Z, ls, 1.7, Kb, torch.zeros(d + 1 + M * d, dtype=torch.float64), kernel, want_gz=True)
    R.assert_close(got, R.pack(g, True), R.pack(A, True), tau=1e-14, what="oracle engine")


# ---- the comparison must notice one missing element ----------------------------------------------------------------------
def _mutation_problem():
    N, M, d, kernel = 1000, 129, 5, "matern32"
    X, y, Z, ls, Pb, bb = small(N, M, d, 21)
    g, A = R.bwd_reference(X, y, Z, ls, 1.7, Pb, bb, -0.7, kernel)
    P = R._ld(Pb)
    last_row = R._contract(R._ld(X[-1:]), R._ld(Z), R._ls(ls, d), R.LD(1.7), P + P.T, np.abs(P) + np.abs(P).T, R._ld(bb), R._ld(y[-1:]),
                           kernel)[0]                                  # what row N - 1 adds, over all columns
    return (N, M, d, kernel), (X, y, Z, ls, Pb, bb), g, A, last_row


def _fails(got, g, A):
    with pytest.raises(AssertionError):
        R.assert_close(got, R.pack(g, True), R.pack(A, True))
    return R.worst_ratio(got, R.pack(g, True), R.pack(A, True))


def test_comparison_notices_one_missing_element():
    """The last valid row times the last valid column: the term a one-off masking error drops."""
    (N, M, d, kernel), (X, y, Z, ls, Pb, bb), g, A, _ = _mutation_problem()
    ldl, P = R._ls(ls, d), R._ld(Pb)
    D = (R._ld(Z) / ldl) - (R._ld(X[-1]) / ldl)[None, :]               # M x d, row N - 1
    kp, hp = R.profile((D * D).sum(-1), kernel)
    kbar = R.LD(1.7) * (kp @ (P + P.T)) + R._ld(y[-1:])[0] * R._ld(bb)  # Kbar_uf[:, N - 1]
    m = M - 1
    e = kbar[m] * R.LD(1.7) * hp[m]
    t_ls, t_sf2, t_z = -2 / ldl * e * D[m] * D[m], kbar[m] * kp[m], 2 / ldl * e * D[m]
    assert abs(t_sf2) > 100 * R.TAU * A["sf2"] and bool((np.abs(t_ls) > 100 * R.TAU * A["ls"]).all())
    assert bool((np.abs(t_z) > 100 * R.TAU * A["Z"][m]).all())
    mut = {"ls": g["ls"] - t_ls, "sf2": g["sf2"] - t_sf2, "Z": g["Z"].copy()}
    mut["Z"][m] -= t_z
    good = R.pack(g, True).astype(np.float64)                          # the reference rounded to float64 passes ...
    assert R.assert_close(good, R.pack(g, True), R.pack(A, True)) < 1e-15
    assert _fails(R.pack(mut, True).astype(np.float64), g, A) > 100 * R.TAU   # ... without the one term it does not
    for key in ("ls", "sf2"):                                          # and each affected output alone gives it away
        one = dict(g)
        one[key] = mut[key]
        _fails(R.pack(one, True).astype(np.float64), g, A)


def test_comparison_notices_one_dimension_of_one_row_left_out():
    (N, M, d, kernel), _, g, A, row = _mutation_problem()
    j = d - 1
    assert abs(row["ls"][j]) > 100 * R.TAU * A["ls"][j]
    mut = {"ls": g["ls"].copy(), "sf2": g["sf2"], "Z": g["Z"].copy()}
    mut["ls"][j] -= row["ls"][j]
    mut["Z"][:, j] -= row["Z"][:, j]
    _fails(R.pack(mut, True).astype(np.float64), g, A)
    only_ls = dict(g)
    only_ls["ls"] = mut["ls"]
    _fails(R.pack(only_ls, True).astype(np.float64), g, A)


def test_comparison_notices_a_missing_kappa_term():
    (N, M, d, kernel), _, g, A, _ = _mutation_problem()
    assert abs(-0.7 * N) > 100 * R.TAU * A["sf2"]
    mut = dict(g)
    mut["sf2"] = g["sf2"] - R.LD(-0.7) * N
    _fails(R.pack(mut, True).astype(np.float64), g, A)
    nan = R.pack(g, True).astype(np.float64)
    nan[3] = float("nan")                                              # an output the call never wrote
    assert R.worst_ratio(nan, R.pack(g, True), R.pack(A, True)) == float("inf")


# ---- the GPU tests' comparison functions, on the oracle engine -----------------------------------------------------------
CPU_CELLS = [(1, 1, 1, "rbf", True), (129, 129, 4, "rbf", True), (255, 130, 5, "matern32", False), (333, 64, 18, "matern32", False),
             (300, 140, 32, "matern52", True)]


@pytest.mark.parametrize("want_gz", [False, True])
@pytest.mark.parametrize("cell", CPU_CELLS, ids=T.cell_id)
def test_gpu_comparison_of_pass2_runs_on_the_oracle_engine(cell, want_gz):
    got, w = T.check_bwd(OracleEngine(), cell, want_gz)
    assert w < 1e-14 and got.numel() == cell[2] + 1 + (cell[1] * cell[2] if want_gz else 0)


def test_gpu_comparison_of_pass2_fails_on_a_wrong_engine():
    class OneRowShort(OracleEngine):
        def suffstats_bwd(self, X, y, Z, *a, **k):
            return super().suffstats_bwd(X[:-1], y[:-1], Z, *a, **k)
    with pytest.raises(AssertionError):
        T.check_bwd(OneRowShort(), (129, 129, 4, "rbf", True), True)


@pytest.mark.parametrize("fcell", [(777, 130, 3, "rbf"), (300, 131, 18, "matern32")], ids=T.cell_id)
def test_gpu_comparison_of_the_factored_mode_runs_on_the_oracle_engine(fcell):
    eng = FactoredOracleEngine()
    assert T.check_factored(eng, fcell) < 1e-13
    assert eng.calls["suffstats_bwd_factored"] == 4 and eng.calls["t_handed_over"] == 2


@pytest.mark.parametrize("kcell", [(1, 1, "rbf"), (2, 8, "matern32"), (257, 18, "matern52"), (130, 32, "rbf")], ids=lambda c: "%d-%d-%s" % c)
def test_gpu_comparison_of_kuu_bwd_runs_on_the_oracle_engine(kcell):
    assert T.check_kuu(OracleEngine(), kcell) < 1e-14
