"""GPU: sgp_exact_eval_batch (csrc/sgp_exact_batch.hip) against the long-double reference at the edge shapes of its three size classes,
the batch plumbing bit for bit, the failure paths, the single-call path, and ``lml_surface`` / ``fit_ml2`` end to end against the
scikit-learn fixtures."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import dev
from exact_batch_reference import TAU, ratios, reference
from pass2_reference import _ld, profile
from exact_batch_double import ExactBatchDouble
from test_exact_batch import bad_theta_rows, check_ml2, check_surface, load, ml2_cells, surface_theta

import ggp_amd

pytestmark = pytest.mark.gpu

NS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]  # small class <= 32 < middle <= 64 < large
DS = [1, 2, 8]
KS = ["rbf", "matern32", "matern52"]
# three cells per N: every d at every N, and the kernel rotated so that every kernel meets every N -- hence every d and every kernel
# at the small, the middle and the large class (39 cells)
CELLS = [(N, DS[k], KS[(i + k) % 3]) for i, N in enumerate(NS) for k in range(3)]


def bits(*tensors):
    return np.concatenate([t.detach().cpu().contiguous().view(-1).numpy().view(np.uint64 if t.dtype == torch.float64 else np.uint32)
                           .astype(np.uint64) for t in tensors])


def spread_theta(X, kernel, P=7):
    """P rows of theta whose matrices run from cond 2 to 1e7 (one decade and a sixth per row).  With the unit-amplitude kernel matrix's
    extreme eigenvalues mu, cond(sf2 k' + s2 I) = (s2 + sf2 mu_max) / (s2 + sf2 mu_min) grows with sf2 towards mu_max / mu_min: the even
    rows take a lengthscale of 1e5 sqrt(d) (k' almost of rank one, any cond within reach already at N = 2), the odd rows an ARD
    lengthscale around 3 sqrt(d) (a full-rank k'); sf2 is solved for the row's target, or left at 1e3 s2 where the target is out of reach."""
    N, d = X.shape
    th = np.zeros((P, d + 2))
    for p in range(P):
        s2 = [1.0, 0.1, 9.0, 0.5, 2.0, 0.1, 1.0][p]
        ls = (1e5 if p % 2 == 0 else 3.0) * np.sqrt(d) * (1.0 + 0.1 * np.arange(d))
        diff = (X[:, None, :] - X[None, :, :]) / ls
        mu = np.linalg.eigvalsh(np.asarray(profile(_ld((diff * diff).sum(-1)), kernel)[0], dtype=np.float64))
        target = max(10.0 ** (7.0 * p / (P - 1)), 2.0)
        room = mu[-1] - target * max(mu[0], 0.0)
        th[p, :d], th[p, d + 1] = ls, s2
        th[p, d] = s2 * (target - 1.0) / room if room > 1e-3 * mu[-1] else 1e3 * s2
    return th


@pytest.mark.parametrize("N,d,kernel", CELLS)
def test_edge_shapes_match_the_long_double_reference(engine, N, d, kernel):
    rng = np.random.default_rng(1000 * N + d)
    X = rng.uniform(0.0, 10.0, (N, d))
    y = 3.0 * rng.standard_normal(N)
    th = spread_theta(X, kernel)
    Xd, yd, thd = dev(X, engine), dev(y, engine), dev(th, engine)
    F, out, g, info = engine.exact_eval_batch(Xd, yd, thd, kernel=kernel)
    F0, out0, g0, info0 = engine.exact_eval_batch(Xd, yd, thd, kernel=kernel, want_grad=False)
    assert g0 is None and int(info.abs().sum()) == 0 and int(info0.abs().sum()) == 0
    assert np.array_equal(bits(out[:, :3]), bits(out0[:, :3])), "the value differs between the two modes"
    assert bool(out0[:, 3].isnan().all())
    Fh, outh, gh = F.cpu().numpy(), out.cpu().numpy(), g.cpu().numpy()
    conds = []
    for p in range(th.shape[0]):
        ref = reference(X, y, th[p, :d], th[p, d], th[p, d + 1], kernel)
        rF, rg = ratios(Fh[p], gh[p], ref)
        print("N=%d d=%d %s p=%d cond %.2e: |dF|/S_F %.2e, |dg|/(cond S_g) %.2e" % (N, d, kernel, p, ref["cond"], rF, rg))
        assert rF <= TAU and rg <= TAU, (p, ref["cond"], rF, rg)
        assert abs(outh[p, 1] - float(ref["quad"])) <= TAU * float(ref["S_F"]) * 2
        assert abs(outh[p, 2] - float(ref["logdet"])) <= TAU * float(ref["S_F"]) * 2
        assert abs(outh[p, 3] - float(ref["trinv"])) <= TAU * ref["cond"] * float(ref["S_g"][-1]) * 2  # S_g[s2] = sum |A^-1|_ii / 2 + ...
        conds.append(ref["cond"])
    if N > 1:
        assert min(conds) < 10.0 and 1e6 <= max(conds) <= 1e8, conds


def plumbing_problem(P, seed=5):
    rng = np.random.default_rng(seed)
    N, d, nX, nY = 33, 2, 3, 5
    X = rng.uniform(0.0, 10.0, (nX, N, d))
    Y = rng.standard_normal((nY, N))
    th = np.exp(rng.uniform(-1.0, 1.5, (P, d + 2)))
    ix = rng.integers(0, nX, P).astype(np.int32)
    iy = rng.integers(0, nY, P).astype(np.int32)
    return X, Y, th, ix, iy


@pytest.mark.parametrize("P", [1, 2, 600])
def test_every_problem_of_a_batch_equals_the_problem_alone(engine, P):
    X, Y, th, ix, iy = plumbing_problem(P)
    Xd, Yd, thd = dev(X, engine), dev(Y, engine), dev(th, engine)
    F, out, g, info = engine.exact_eval_batch(Xd, Yd, thd, ix=ix, iy=iy, kernel="matern52")
    assert int(info.abs().sum()) == 0
    whole = np.concatenate([bits(out).reshape(P, 4), bits(g).reshape(P, -1)], 1)
    for p in range(P):
        _, o1, g1, i1 = engine.exact_eval_batch(Xd[ix[p]].contiguous(), Yd[iy[p]].contiguous(), thd[p:p + 1].contiguous(),
                                                kernel="matern52")
        assert np.array_equal(np.concatenate([bits(o1), bits(g1)]), whole[p]), p
    # the host-side range check of a host index list
    with pytest.raises(ValueError):
        engine.exact_eval_batch(Xd, Yd, thd, ix=[3] * P, iy=iy)


def test_same_bits_on_every_launch_context_and_stream():
    X, Y, th, ix, iy = plumbing_problem(64, seed=6)
    e0 = ggp_amd.HipEngine()
    Xd, Yd, thd = dev(X, e0), dev(Y, e0), dev(th, e0)

    def run(eng, stream=None):
        if stream is None:
            r = eng.exact_eval_batch(Xd, Yd, thd, ix=ix, iy=iy)
        else:
            with torch.cuda.stream(stream):
                r = eng.exact_eval_batch(Xd, Yd, thd, ix=ix, iy=iy)
            stream.synchronize()
        return bits(r[1], r[2], r[3])

    first = run(e0)
    for _ in range(19):
        assert np.array_equal(run(e0), first)
    a, b = ggp_amd.HipEngine(own_context=True), ggp_amd.HipEngine(own_context=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    assert np.array_equal(run(a, sa), first) and np.array_equal(run(b, sb), first)


def test_one_singular_problem_leaves_its_neighbours_alone(engine):
    rng = np.random.default_rng(2)
    N, d = 40, 3
    X = rng.standard_normal((2, N, d))
    X[1, 20:] = X[1, :20]  # duplicated rows
    y = rng.standard_normal(N)
    th = np.exp(rng.uniform(-0.5, 0.5, (9, d + 2)))
    ix = np.zeros(9, dtype=np.int32)
    th[4] = [1.0, 1.0, 1.0, 1.0, 1e-300]
    ix[4] = 1
    Xd, yd = dev(X, engine), dev(y, engine)
    F, out, g, info = engine.exact_eval_batch(Xd, yd, dev(th, engine), ix=ix)
    keep = [p for p in range(9) if p != 4]
    F8, out8, g8, info8 = engine.exact_eval_batch(Xd, yd, dev(th[keep], engine), ix=ix[keep])
    info = info.cpu().numpy()
    assert info[4] != 0 and not info[keep].any() and not info8.cpu().numpy().any()
    assert bool(out[4].isnan().all()) and bool(g[4].isnan().all())
    idx = torch.as_tensor(keep, device=engine.device)
    assert np.array_equal(bits(out[idx], g[idx]), bits(out8, g8))


def test_a_theta_that_is_not_positive_and_finite_is_reported_like_the_double(engine):
    """A negative lengthscale, sf2 = 0 or a negative sf2 under a large s2 would pass the factorisation: the kernel tests theta itself."""
    rng = np.random.default_rng(4)
    X, y = rng.uniform(0, 10, (6, 2)), rng.standard_normal(6)
    th = bad_theta_rows()
    Xd, yd = dev(X, engine), dev(y, engine)
    _, _, _, want = ExactBatchDouble().exact_eval_batch(X, y, th)
    for want_grad in (True, False):
        F, out, g, info = engine.exact_eval_batch(Xd, yd, dev(th, engine), want_grad=want_grad)
        assert info.cpu().tolist() == want.tolist() == [0] + [1] * 7
        assert bool(out[1:].isnan().all()) and (g is None or bool(g[1:].isnan().all()))
        _, out1, g1, _ = engine.exact_eval_batch(Xd, yd, dev(th[:1], engine), want_grad=want_grad)
        assert np.array_equal(bits(out[:1, :3]), bits(out1[:, :3])) and (g is None or np.array_equal(bits(g[:1]), bits(g1)))
    got = ggp_amd.lml_surface(X, y, th[:, 2], th[:, :2], th[:, 3], engine=engine)
    assert np.isfinite(got[0]) and np.isnan(got[1:]).all()


def test_occupancy_query(engine):
    lib = engine.lib
    for k in range(3):
        small, middle, large = (lib.sgp_exact_batch_occupancy(N, k) for N in (32, 64, 128))
        print("kernel %d: workgroups per CU %d / %d / %d" % (k, small, middle, large))
        assert small >= middle >= large == 1  # the large class's image is 141 KiB of the CU's 160 KiB of LDS: one workgroup
    assert lib.sgp_exact_batch_occupancy(129, 0) == -2 and lib.sgp_exact_batch_occupancy(0, 0) == -1
    assert lib.sgp_exact_batch_occupancy(10, 3) == -1


def test_out_of_range_arguments_are_refused(engine):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=engine.device)  # noqa: E731
    for X, Y, th, kw, status in ((z(129, 1), z(129), z(2, 3), {}, -2), (z(10, 9), z(10), z(2, 11), {}, -2),
                                 (z(10, 2), z(10), z(2, 4), {"kernel": "composite"}, -1), (z(10, 2), z(10), z(0, 4), {}, -1)):
        with pytest.raises(ggp_amd.SgpStatusError) as ei:
            engine.exact_eval_batch(X, Y, th, **kw)
        assert ei.value.status == status
    lib = engine.lib
    assert lib.sgp_exact_batch_workspace_bytes(4, 129, 1, 1) == 0 and lib.sgp_exact_batch_workspace_bytes(4, 10, 9, 1) == 0
    assert lib.sgp_exact_batch_workspace_bytes(0, 10, 1, 1) == 0
    need = lib.sgp_exact_batch_workspace_bytes(2, 10, 2, 1)
    assert need > 0
    X, Y, th = z(10, 2), z(10), torch.ones(2, 4, dtype=torch.float64, device=engine.device)
    out, g = z(2, 4), z(2, 4)
    info = torch.zeros(2, dtype=torch.int32, device=engine.device)
    ws = torch.empty(need, dtype=torch.uint8, device=engine.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda ws_ptr, nbytes, P=2: (p(X), 20, 2, p(Y), 10, None, None, p(th), P, 10, 2, 0, 1, p(out), p(g), p(info), ws_ptr, nbytes,  # noqa: E731
                                        engine._stream())
    assert lib.sgp_exact_eval_batch(*args(p(ws), need - 1)) == -3
    assert lib.sgp_exact_eval_batch(*args(None, need)) == -3
    # P x 256 work-items must stay below the 2^32 of one launch: P = 2^24 is refused here, not by the runtime after the launch
    assert lib.sgp_exact_batch_workspace_bytes(2 ** 24, 10, 2, 1) == 0 and lib.sgp_exact_batch_workspace_bytes(2 ** 24 - 1, 10, 2, 1) > 0
    assert lib.sgp_exact_eval_batch(*args(p(ws), need, P=2 ** 24)) == -2
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # nothing was enqueued: the output is untouched
    assert lib.sgp_exact_eval_batch(*args(p(ws), need)) == 0
    torch.cuda.synchronize()
    assert bool(out[:, 0].isfinite().all())


@pytest.mark.parametrize("N", [30, 120])
def test_batch_agrees_with_the_single_call_path(engine, N):
    rng = np.random.default_rng(N)
    d = 2
    X = rng.uniform(0.0, 10.0, (N, d))
    y = 3.0 * rng.standard_normal(N)
    th = np.array([[1.5, 2.5, 25.0, 1.0], [4.0, 3.0, 2.0, 0.1], [0.7, 0.9, 1.0, 0.3]])
    Xd, yd = dev(X, engine), dev(y, engine)
    F, out, g, info = engine.exact_eval_batch(Xd, yd, dev(th, engine))
    Fh, gh = F.cpu().numpy(), g.cpu().numpy()
    for p in range(3):
        r = engine.exact_eval(Xd, yd, list(th[p, :d]), th[p, d], th[p, d + 1])
        ref = reference(X, y, th[p, :d], th[p, d], th[p, d + 1])
        assert r["info"] == 0
        assert abs(r["F"] - Fh[p]) <= 2 * TAU * float(ref["S_F"])
        single = np.array(r["ls"] + [r["sf2"], r["s2"]])
        lim = 2 * TAU * ref["cond"] * np.asarray(ref["S_g"], dtype=np.float64)
        assert (np.abs(single - gh[p]) <= lim).all(), (single, gh[p], lim)


@pytest.mark.parametrize("name", ["a", "b"])
def test_lml_surface_matches_sklearn_on_the_device(engine, name):
    G = load("lml_surface")
    sf2, ls, s2 = surface_theta(G, name)
    check_surface(ggp_amd.lml_surface(G[name + "_X"], G[name + "_y"], sf2[:, None], ls[None, :], s2, engine=engine), G, name)


@pytest.mark.parametrize("c", [1, 2])  # (10, learn) and (40, learn)
def test_fit_ml2_on_the_device_is_no_worse_than_sklearn(engine, c):
    cell = ml2_cells()[c]
    assert str(cell["noise"]) == "learn" and cell["X"].shape[0] in (10, 40)
    res = ggp_amd.fit_ml2(cell["X"], cell["Y"], noise="learn", theta0=cell["theta0"], bounds=cell["bounds"], starts=cell["starts"],
                          engine=engine)
    check_ml2(res, cell)
