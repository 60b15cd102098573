"""The batched collapsed bound (csrc/sgp_vfe_batch.hip: sgp_vfe_eval_batch, one workgroup per problem) against the long-double
reference tests/vfe_reference.py, and the Python layer on it (``elbo_surface``, ``fit_sgpr_batch``) on the device.

Cells (tests/vfe_batch_double.py, named N-M-d-kernel[-tag]): those of ``vfe_reference.CELLS`` the kernel can take -- the 16-column
panels (M = 15 | 16 | 17, 48 | 49, 63 | 64), M > N, the ill-conditioned ones -- and nine of its own for what is new here: the size classes
Mp = 16 | 32 | 64 at their edges (M = 1, 16, 31 | 32 | 33, 64), d = 8, and more than one row tile in every class.  The tiles are 128, 64
and 32 rows: the small class walks several of them at 257-16-2 (a last tile of one row), 129-1-1 and 256-9-3 (two full tiles) -- its
four waves split the rows of a tile in pass 1 --, the middle class at 1984 | 1985-17-2 and 200-33-2, the large one at 129-48-3 to 2049-64-3.

Every entry of out (value, all gradients, logmarg, trace) and of dF/dZ is compared component-wise:

    |got - ref| <= MARGIN * max(e64, FLOOR) * scale,   MARGIN = 10, FLOOR = 1e-13   (vfe_reference's own)

scale the reference's condition scale of that component, e64 the float64 level of the cell and output group: the worse of two float64
evaluations of the closed form against long double, measured on the CPU (``vfe_batch_double.measure_e64``) and written below to one
significant digit; tests/test_vfe_batch.py recomputes the table and shows deliberate defects failing the comparison.  At each cell
also: info == 0, the value-only call returns the same F, logmarg and trace bit for bit, a second call returns the same bits, and the
workspace (a placeholder the kernel never touches, include/sgp_vfe_batch.h) is filled with 0xFF bytes before the launch.
"""

import numpy as np
import pytest
import torch

import vfe_batch_double as D
import vfe_reference as V
from conftest import dev

# --- table (measured on the CPU, one significant digit) ---
E64 = {
    "1-1-1-rbf": {"F": 4e-17, "g_ls": 0.0, "g_sf2": 2e-17, "g_s2": 3e-17, "logmarg": 6e-17, "trace": 9e-17, "g_Z": 0.0},
    "63-15-2-rbf": {"F": 2e-16, "g_ls": 2e-16, "g_sf2": 1e-16, "g_s2": 2e-16, "logmarg": 6e-17, "trace": 4e-16, "g_Z": 2e-15},
    "64-16-2-matern32": {"F": 6e-17, "g_ls": 2e-16, "g_sf2": 2e-16, "g_s2": 2e-17, "logmarg": 1e-16, "trace": 3e-17, "g_Z": 2e-15},
    "65-17-2-rbf": {"F": 8e-16, "g_ls": 3e-16, "g_sf2": 2e-17, "g_s2": 8e-16, "logmarg": 5e-16, "trace": 1e-15, "g_Z": 2e-14},
    "129-48-3-matern52": {"F": 2e-17, "g_ls": 2e-16, "g_sf2": 3e-16, "g_s2": 2e-17, "logmarg": 5e-17, "trace": 1e-17, "g_Z": 4e-15},
    "130-49-1-rbf": {"F": 1e-15, "g_ls": 2e-15, "g_sf2": 7e-17, "g_s2": 1e-15, "logmarg": 2e-15, "trace": 3e-15, "g_Z": 2e-13},
    "200-63-2-rbf": {"F": 8e-16, "g_ls": 6e-16, "g_sf2": 7e-16, "g_s2": 9e-16, "logmarg": 7e-16, "trace": 2e-15, "g_Z": 9e-14},
    "200-64-2-matern32": {"F": 3e-16, "g_ls": 1e-16, "g_sf2": 1e-16, "g_s2": 2e-16, "logmarg": 1e-16, "trace": 4e-16, "g_Z": 4e-14},
    "40-60-2-rbf": {"F": 4e-15, "g_ls": 7e-16, "g_sf2": 3e-17, "g_s2": 3e-15, "logmarg": 1e-15, "trace": 7e-15, "g_Z": 1e-13},
    "1984-17-2-rbf": {"F": 7e-15, "g_ls": 5e-16, "g_sf2": 4e-17, "g_s2": 6e-15, "logmarg": 2e-16, "trace": 1e-14, "g_Z": 1e-14},
    "1985-17-2-rbf": {"F": 4e-15, "g_ls": 4e-16, "g_sf2": 9e-17, "g_s2": 3e-15, "logmarg": 1e-16, "trace": 5e-15, "g_Z": 5e-15},
    "200-64-2-rbf-ill": {"F": 7e-16, "g_ls": 6e-17, "g_sf2": 1e-17, "g_s2": 1e-15, "logmarg": 8e-15, "trace": 2e-15, "g_Z": 5e-14},
    "200-33-2-matern32-near": {"F": 9e-15, "g_ls": 2e-16, "g_sf2": 7e-17, "g_s2": 9e-15, "logmarg": 2e-14, "trace": 2e-14, "g_Z": 2e-11},
    "200-64-2-rbf-sf100": {"F": 1e-12, "g_ls": 1e-16, "g_sf2": 2e-17, "g_s2": 2e-12, "logmarg": 1e-12, "trace": 2e-12, "g_Z": 2e-12},
    "17-31-2-rbf": {"F": 8e-17, "g_ls": 4e-16, "g_sf2": 1e-16, "g_s2": 8e-17, "logmarg": 1e-16, "trace": 2e-16, "g_Z": 1e-13},
    "33-32-8-matern52": {"F": 4e-17, "g_ls": 1e-15, "g_sf2": 2e-16, "g_s2": 5e-17, "logmarg": 5e-17, "trace": 5e-17, "g_Z": 8e-15},
    "257-33-8-rbf": {"F": 6e-17, "g_ls": 6e-16, "g_sf2": 3e-16, "g_s2": 9e-17, "logmarg": 1e-16, "trace": 2e-17, "g_Z": 2e-15},
    "2049-64-3-matern32": {"F": 6e-17, "g_ls": 1e-16, "g_sf2": 7e-17, "g_s2": 9e-17, "logmarg": 4e-17, "trace": 6e-17, "g_Z": 2e-15},
    "16-1-1-matern52": {"F": 3e-17, "g_ls": 5e-16, "g_sf2": 1e-16, "g_s2": 1e-17, "logmarg": 7e-17, "trace": 3e-17, "g_Z": 5e-17},
    "257-16-2-rbf": {"F": 2e-15, "g_ls": 4e-16, "g_sf2": 4e-17, "g_s2": 1e-15, "logmarg": 1e-16, "trace": 2e-15, "g_Z": 2e-14},
    "129-1-1-matern52": {"F": 7e-18, "g_ls": 2e-16, "g_sf2": 7e-17, "g_s2": 6e-17, "logmarg": 4e-17, "trace": 4e-17, "g_Z": 1e-16},
    "256-9-3-matern32": {"F": 5e-17, "g_ls": 4e-16, "g_sf2": 1e-16, "g_s2": 5e-17, "logmarg": 1e-16, "trace": 3e-17, "g_Z": 1e-15},
    "100-64-1-rbf": {"F": 3e-15, "g_ls": 5e-16, "g_sf2": 2e-17, "g_s2": 3e-15, "logmarg": 1e-15, "trace": 4e-15, "g_Z": 4e-13},
}
# --- end of table ---
FLOOR_E64 = {k: 0.0 for k in D.GROUPS}   # problems outside the table: the FLOOR sets the tolerance (test_vfe_batch.py measures them)


def check(what, got, ref, A, e64, keys=D.GROUPS):
    """Prints every group's worst |got - ref| / scale beside its tolerance, then asserts.  Returns {group: ratio}."""
    w = V.worst(got, ref, A, keys)
    tol = {k: V.tolerance(e64[k]) for k in keys}
    print("VFE_BATCH %s  %s" % (what, "  ".join("%s %.2g/%.0e" % (k, w[k], tol[k]) for k in keys)))
    bad = {k: (w[k], tol[k]) for k in keys if not w[k] <= tol[k]}
    assert not bad, (what, bad)
    return w


def poison(engine):
    """0xFF bytes over the workspace the next launch is handed."""
    ws = engine._workspace("vfe_batch", 256)
    ws.fill_(0xFF)
    return ws


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def launch(engine, name, want_grad=True):
    inp = D.inputs(name)
    X, y, Z, th = dev(inp["X"], engine), dev(inp["y"], engine), dev(inp["Z"], engine), dev(inp["theta"][None], engine)
    poison(engine)
    out, gz, info = engine.vfe_eval_batch(X, y, Z, th, kernel=inp["kernel"], jitter=inp["jitter"], want_grad=want_grad, want_gz=want_grad)
    return out[0].cpu().clone(), (gz[0].cpu().clone() if gz is not None else None), int(info.item())


@pytest.mark.gpu
@pytest.mark.parametrize("name", D.CELLS)
def test_batched_bound_against_the_long_double_reference(engine, name):
    d = D.spec(name)["d"]
    out, gz, info = launch(engine, name)
    assert info == 0
    check(name, D.unpack(out.numpy(), gz.numpy(), d), *D.reference(name), E64[name])
    out1, gz1, info1 = launch(engine, name, want_grad=False)
    assert info1 == 0 and gz1 is None and bool(out1[1:d + 3].isnan().all())
    assert same_bits(out1[[0, d + 3, d + 4]], out[[0, d + 3, d + 4]])   # the value-only call: F, logmarg, trace bit for bit
    out2, gz2, info2 = launch(engine, name)
    assert info2 == 0 and same_bits(out2, out) and same_bits(gz2, gz)


# ---------------------------------------------------------------------------------------------------------------- heterogeneous batch
def hetero_problem(seed=5):
    """P = 37 problems over 3 data sets x 2 targets x 3 inducing sets at (N, M, d) = (65, 17, 2), with distinct theta rows."""
    rng = np.random.default_rng(seed)
    N, M, d, P = 65, 17, 2, 37
    X = rng.standard_normal((3, N, d))
    Y = np.stack([np.sin(X[0].sum(1)), np.cos(X[1, :, 0])]) + 0.1 * rng.standard_normal((2, N))
    Z = np.stack([X[s][rng.permutation(N)[:M]] for s in range(3)])
    theta = np.exp(np.concatenate([rng.uniform(np.log(0.6), np.log(1.6), (P, d)), rng.uniform(np.log(0.5), np.log(2.0), (P, 1)),
                                   rng.uniform(np.log(0.03), np.log(0.3), (P, 1))], 1))
    ix, iy, iz = rng.integers(0, 3, P), rng.integers(0, 2, P), rng.integers(0, 3, P)
    return X, Y, Z, theta, ix, iy, iz


@pytest.mark.gpu
def test_heterogeneous_batch_bits_do_not_depend_on_the_batch(engine):
    X, Y, Z, theta, ix, iy, iz = hetero_problem()
    Xd, Yd, Zd, thd = (dev(a, engine) for a in (X, Y, Z, theta))
    P, d = theta.shape[0], X.shape[2]
    call = lambda rows: engine.vfe_eval_batch(Xd, Yd, Zd, thd[rows].contiguous(), ix=ix[rows], iy=iy[rows], iz=iz[rows], kernel="matern52",  # noqa: E731
                                              jitter=1e-6, want_grad=True, want_gz=True)
    poison(engine)
    out, gz, info = call(np.arange(P))
    assert int(info.abs().sum()) == 0 and bool(out.isfinite().all()) and bool(gz.isfinite().all())
    for p in range(P):   # alone
        o1, g1, i1 = call(np.array([p]))
        assert int(i1.item()) == 0 and same_bits(o1[0], out[p]) and same_bits(g1[0], gz[p]), p
    rows = np.array([30, 7, 36, 0, 19])   # at another position in a P = 5 call
    o5, g5, i5 = call(rows)
    assert int(i5.abs().sum()) == 0 and same_bits(o5, out[rows]) and same_bits(g5, gz[rows])
    for p in (0, 7, 19, 30, 36):   # against the reference (e64 of these well-conditioned problems lies below the FLOOR: test_vfe_batch.py)
        ref, A = V.stationary(X[ix[p]], Y[iy[p]], Z[iz[p]], theta[p, :d], theta[p, d], theta[p, d + 1], 1e-6, "matern52")
        check("hetero %d" % p, D.unpack(out[p].cpu().numpy(), gz[p].cpu().numpy(), d), ref, A, FLOOR_E64)
    # a second stream, and the plain entry point beside the context twin
    side = torch.cuda.Stream(device=engine.device)
    side.wait_stream(torch.cuda.current_stream(engine.device))
    with torch.cuda.stream(side):
        o_s, g_s, i_s = call(np.arange(P))
    side.synchronize()
    assert same_bits(o_s, out) and same_bits(g_s, gz) and int(i_s.abs().sum()) == 0
    lib = engine.vfe_batch_lib
    o_c, g_c = engine.empty(P, d + 5), engine.empty(P, 17, d)
    i_c = torch.empty(P, dtype=torch.int32, device=engine.device)
    ws = poison(engine)
    ixd, iyd, izd = (torch.as_tensor(a.astype(np.int32), device=engine.device) for a in (ix, iy, iz))
    p_ = engine._ptr
    args = (p_(Xd), 65 * d, d, p_(Yd), 65, p_(ixd), p_(iyd), p_(Zd), 17 * d, d, p_(izd), p_(thd), P, 65, 17, d, 2, 1e-6, 1, p_(o_c), p_(g_c),
            p_(i_c), p_(ws), ws.numel(), engine._stream())
    assert lib.sgp_vfe_eval_batch(*args) == 0
    torch.cuda.synchronize()
    assert same_bits(o_c, out) and same_bits(g_c, gz)
    o_c.zero_()
    assert lib.sgp_ctx_vfe_eval_batch(None, *args) == 0
    torch.cuda.synchronize()
    assert same_bits(o_c, out) and same_bits(g_c, gz)
    # padded leading dimensions and set strides (NaN in the padding, which must never be read): the same bits
    ldx, ldz, xs, ys, zs = 5, 3, 65 * 5 + 7, 65 + 3, 17 * 3 + 2
    Xp, Yp, Zp = np.full((3, xs), np.nan), np.full((2, ys), np.nan), np.full((3, zs), np.nan)
    for s_ in range(3):
        Xp[s_, :65 * ldx].reshape(65, ldx)[:, :d] = X[s_]
        Zp[s_, :17 * ldz].reshape(17, ldz)[:, :d] = Z[s_]
    Yp[:, :65] = Y
    Xq, Yq, Zq = dev(Xp, engine), dev(Yp, engine), dev(Zp, engine)
    o_c.zero_(), g_c.zero_()
    padded = (p_(Xq), xs, ldx, p_(Yq), ys, p_(ixd), p_(iyd), p_(Zq), zs, ldz, p_(izd)) + args[11:]
    assert lib.sgp_vfe_eval_batch(*padded) == 0
    torch.cuda.synchronize()
    assert int(i_c.abs().sum()) == 0 and same_bits(o_c, out) and same_bits(g_c, gz)


# ---------------------------------------------------------------------------------------------------------------- failures stay local
@pytest.mark.gpu
def test_failures_stay_local(engine):
    X, Y, Z, theta, ix, iy, iz = hetero_problem(seed=6)
    P, d, M = 8, 2, 17
    theta, ix, iy, iz = theta[:P].copy(), ix[:P], iy[:P], iz[:P].copy()
    Zdup = Z[0].copy()
    Zdup[1] = Zdup[0]   # two identical inducing inputs: K_uu is singular without a jitter
    Z4 = np.concatenate([Z, Zdup[None]])
    Xd, Yd, Zd = dev(X, engine), dev(Y, engine), dev(Z4, engine)
    call = lambda th, iz_: engine.vfe_eval_batch(Xd, Yd, Zd, dev(th, engine), ix=ix, iy=iy, iz=iz_, kernel="rbf", jitter=0.0,  # noqa: E731
                                                 want_grad=True, want_gz=True)
    good, good_gz, good_info = call(theta, iz)
    assert int(good_info.abs().sum()) == 0
    cases = {"nan": (1, 0, np.nan), "zero": (2, d, 0.0), "negative": (4, d + 1, -0.3), "inf": (6, 1, np.inf)}
    for what, (p, col, value) in cases.items():
        th = theta.copy()
        th[p, col] = value
        out, gz, info = call(th, iz)
        keep = [q for q in range(P) if q != p]
        assert info.cpu().tolist() == [1 if q == p else 0 for q in range(P)], what
        assert bool(out[p].isnan().all()) and bool(gz[p].isnan().all()), what
        assert same_bits(out[keep], good[keep]) and same_bits(gz[keep], good_gz[keep]), what
    izd = iz.copy()
    izd[3] = 3
    out, gz, info = call(theta, izd)
    keep = [q for q in range(P) if q != 3]
    assert 1 <= int(info[3]) <= M and info[keep].cpu().tolist() == [0] * (P - 1)
    assert bool(out[3].isnan().all()) and bool(gz[3].isnan().all())
    assert same_bits(out[keep], good[keep]) and same_bits(gz[keep], good_gz[keep])
    # value-only: the same report, NaN in the failed row alone
    out0, _, info0 = engine.vfe_eval_batch(Xd, Yd, Zd, dev(theta, engine), ix=ix, iy=iy, iz=izd, kernel="rbf", jitter=0.0, want_grad=False)
    assert info0.cpu().tolist() == info.cpu().tolist() and bool(out0[3].isnan().all()) and same_bits(out0[keep][:, 0], good[keep][:, 0])


# ---------------------------------------------------------------------------------------------------------------- the single launch
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["65-17-2-rbf", "200-64-2-matern32"])
def test_agreement_with_the_single_launch(engine, name):
    """sgp_small_eval and the batched kernel at the same cell: each within its tolerance of the reference (bits are not compared)."""
    import test_small_reference_gpu as S
    d = D.spec(name)["d"]
    out, gz, info = launch(engine, name)
    so, sgz, sinfo = S.launch(engine, name)
    assert info == 0 and sinfo == 0
    ref, A = D.reference(name)
    check("batched " + name, D.unpack(out.numpy(), gz.numpy(), d), ref, A, E64[name])
    S.check("single " + name, V.unpack(name, so.numpy(), sgz.numpy()), ref, A, S.E64[name], V.groups_of(name))


# ---------------------------------------------------------------------------------------------------------------- Python on the device
@pytest.mark.gpu
def test_elbo_surface_equals_the_cells_on_the_device(engine):
    import ggp_amd
    inp = D.inputs("65-17-2-rbf")
    sf2, ls, s2 = np.linspace(0.5, 2.0, 6)[:, None], np.linspace(0.5, 1.5, 5)[None, :], 0.07
    F, lm, tr = ggp_amd.elbo_surface(inp["X"], inp["y"], inp["Z"], sf2, ls, s2, kernel="rbf", jitter=1e-6, parts=True, engine=engine)
    assert F.shape == lm.shape == tr.shape == (6, 5) and np.isfinite(F).all()
    X, y, Z = (dev(inp[k], engine) for k in ("X", "y", "Z"))
    for i in range(6):
        for j in range(5):
            th = dev(np.array([[ls[0, j], ls[0, j], sf2[i, 0], s2]]), engine)
            out, _, info = engine.vfe_eval_batch(X, y, Z, th, kernel="rbf", jitter=1e-6, want_grad=False)
            o = out[0].cpu().numpy()
            assert int(info.item()) == 0 and (F[i, j], lm[i, j], tr[i, j]) == (o[0], o[5], o[6]), (i, j)


def fit_data(B=3, N=60, M=8, seed=11):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-3.0, 3.0, (B, N, 1)), 1)
    Y = np.sin(2.0 * X[:, :, 0]) * np.array([1.0, 0.5, 2.0])[:B, None] + 0.2 * rng.standard_normal((B, N))
    Z = np.stack([np.linspace(-2.5, 2.5, M)[:, None]] * B)
    return X, Y, Z


@pytest.mark.gpu
def test_fit_sgpr_batch_on_the_device(engine):
    import ggp_amd
    from ggp_amd.core import CollapsedBound
    X, Y, Z = fit_data()
    fit = ggp_amd.fit_sgpr_batch(X, Y, Z, n_restarts=1, max_steps=40, lr=0.05, seed=3, engine=engine)
    assert fit.losses.shape == (40, 3, 2) and fit.n_launches == 41 and int(fit.n_bad_steps.sum()) == 0
    alone = ggp_amd.fit_sgpr_batch(X[0], Y[0], Z[0], n_restarts=1, max_steps=40, lr=0.05, seed=3, engine=engine)
    assert np.array_equal(alone.losses[:, 0].view(np.int64), fit.losses[:, 0].view(np.int64))   # the trajectory, bit for bit
    assert np.array_equal(alone.theta_all[0].view(np.int64), fit.theta_all[0].view(np.int64))
    assert np.array_equal(alone.Z_all[0].view(np.int64), fit.Z_all[0].view(np.int64))
    N = X.shape[1]
    assert (fit.elbo_all >= -N * fit.losses[0]).all()   # final F >= initial F for every problem
    assert np.array_equal(fit.elbo, fit.elbo_all.max(1))
    # the fitted model evaluates the same bound through the multi-launch CollapsedBound
    b = 1
    m = fit.model(b)
    d = 1
    ls, sf2, s2 = m._hypers()
    assert np.allclose(ls + [sf2, s2], fit.theta[b], rtol=1e-12)
    cb = m._bound()
    assert isinstance(cb, CollapsedBound) and cb.jitter == 1e-6
    F_cb, parts = cb.value(m.inducing_points, ls, sf2, s2)
    assert parts["info"] == 0
    for what, got, th in (("batched", fit.elbo[b], fit.theta[b]), ("CollapsedBound", F_cb, np.array(ls + [sf2, s2]))):
        args = (X[b], Y[b], fit.Z[b], th[:d], th[d], th[d + 1], 1e-6, "rbf")
        ref, A = V.stationary(*args, grads=False)
        e64 = max(abs(float(V.stationary(*args, np.float64, order, grads=False)[0]["F"] - ref["F"])) for order in ("inverse", "substitution"))
        tol = V.tolerance(e64 / float(A["F"])) * float(A["F"])
        print("VFE_BATCH fitted F through %s: |got - ref| %.2g, tolerance %.2g" % (what, abs(got - float(ref["F"])), tol))
        assert abs(got - float(ref["F"])) <= tol, what
    mean = m.posterior_predictive(torch.as_tensor(X[b, :5], device=engine.device)).mean
    assert mean.shape == (5,) and bool(torch.isfinite(mean).all())
