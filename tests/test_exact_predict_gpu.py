"""GPU: sgp_exact_predict_batch and sgp_exact_mixture_reduce (csrc/sgp_exact_predict.hip) against the long-double reference at the edge
shapes of the three size classes and across the 16-point test tile, the batch plumbing bit for bit, the failure paths, the single-call
path, the reduction under its derived bounds, the refusals, and ``ExactNutsResult.predict`` / ``Ml2Result.predict`` end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import dev
from exact_predict_reference import EPS, TAU, reference
from test_exact_batch import bad_theta_rows
from test_exact_batch_gpu import bits, plumbing_problem
from test_exact_predict import CELLS_A, CELLS_B, check_edge_cell, check_mixture, check_t_edges

import ggp_amd

pytestmark = pytest.mark.gpu


# (a)
@pytest.mark.parametrize("N,d,kernel", CELLS_A)
def test_edge_shapes_match_the_long_double_reference(engine, N, d, kernel):
    worst = check_edge_cell(engine, lambda a: dev(a, engine), N, d, kernel)
    print("N=%d d=%d %s: worst |dmu|/S_mu %.3e, |dv|/S_v %.3e" % (N, d, kernel, worst[0], worst[1]))


# (b)
@pytest.mark.parametrize("N,d", CELLS_B)
def test_t_edges_meet_the_bound_with_the_bits_of_the_long_call(engine, N, d):
    check_t_edges(engine, lambda a: dev(a, engine), N, d, same_bits=True)


# (c)
def predict_problem(P, seed=5, T=19):
    X, Y, th, ix, iy = plumbing_problem(P, seed)
    rng = np.random.default_rng(seed + 100)
    Xs = rng.uniform(0.0, 10.0, (2, T, X.shape[2]))
    return X, Y, Xs, th, ix, iy, rng.integers(0, 2, P).astype(np.int32)


@pytest.mark.parametrize("P", [1, 2, 600])
def test_every_problem_of_a_batch_equals_the_problem_alone(engine, P):
    X, Y, Xs, th, ix, iy, ixs = predict_problem(P)
    Xd, Yd, Xsd, thd = dev(X, engine), dev(Y, engine), dev(Xs, engine), dev(th, engine)
    mean, var, info = engine.exact_predict_batch(Xd, Yd, thd, Xsd, ix=ix, iy=iy, ixs=ixs, kernel="matern52")
    assert int(info.abs().sum()) == 0
    whole = np.concatenate([bits(mean).reshape(P, -1), bits(var).reshape(P, -1)], 1)
    alone = []
    for p in range(P):
        m1, v1, _ = engine.exact_predict_batch(Xd[ix[p]].contiguous(), Yd[iy[p]].contiguous(), thd[p:p + 1].contiguous(),
                                               Xsd[ixs[p]].contiguous(), kernel="matern52")
        alone.append(torch.cat([m1, v1], 1))
    assert np.array_equal(bits(torch.cat(alone)).reshape(P, -1), whole)
    for kw in ({"ix": [3] * P}, {"iy": [5] * P}, {"ixs": [2] * P}, {"ixs": [-1] * P}):
        with pytest.raises(ValueError):
            engine.exact_predict_batch(Xd, Yd, thd, Xsd, **{**dict(ix=ix, iy=iy, ixs=ixs), **kw})


# (d)
def test_same_bits_on_every_launch_context_and_stream():
    X, Y, Xs, th, ix, iy, ixs = predict_problem(64, seed=6)
    e0 = ggp_amd.HipEngine()
    Xd, Yd, Xsd, thd = dev(X, e0), dev(Y, e0), dev(Xs, e0), dev(th, e0)
    Yt = dev(np.random.default_rng(1).standard_normal((4, Xs.shape[1])), e0)

    def run(eng, stream=None):
        def go():
            m, v, i = eng.exact_predict_batch(Xd, Yd, thd, Xsd, ix=ix, iy=iy, ixs=ixs)
            r = eng.exact_mixture(m, v, i, [0, 1, 3, 40, 64], Ytest=Yt)
            return m, v, i, r["mean"], r["var"], r["logpdf"], r["mean_logpdf"], r["kept"]
        if stream is None:
            out = go()
        else:
            with torch.cuda.stream(stream):
                out = go()
            stream.synchronize()
        return bits(*out)

    first = run(e0)
    for _ in range(19):
        assert np.array_equal(run(e0), first)
    a, b = ggp_amd.HipEngine(own_context=True), ggp_amd.HipEngine(own_context=True)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    assert np.array_equal(run(a, sa), first) and np.array_equal(run(b, sb), first)


# (e)
def test_one_singular_problem_leaves_its_neighbours_alone(engine):
    rng = np.random.default_rng(2)
    N, d, T = 40, 3, 21
    X = rng.standard_normal((2, N, d))
    X[1, 20:] = X[1, :20]  # duplicated rows
    y = rng.standard_normal(N)
    Xs = rng.standard_normal((T, d))
    th = np.exp(rng.uniform(-0.5, 0.5, (9, d + 2)))
    ix = np.zeros(9, dtype=np.int32)
    th[4] = [1.0, 1.0, 1.0, 1.0, 1e-300]
    ix[4] = 1
    Xd, yd, Xsd = dev(X, engine), dev(y, engine), dev(Xs, engine)
    mean, var, info = engine.exact_predict_batch(Xd, yd, dev(th, engine), Xsd, ix=ix)
    keep = [p for p in range(9) if p != 4]
    mean8, var8, info8 = engine.exact_predict_batch(Xd, yd, dev(th[keep], engine), Xsd, ix=ix[keep])
    info_h = info.cpu().numpy()
    assert info_h[4] != 0 and not info_h[keep].any() and not info8.cpu().numpy().any()
    assert bool(mean[4].isnan().all()) and bool(var[4].isnan().all())
    idx = torch.as_tensor(keep, device=engine.device)
    assert np.array_equal(bits(mean[idx], var[idx]), bits(mean8, var8))
    # through the mixture: a group with one failed draw keeps the rest; a group of failed draws alone is NaN; the others are untouched
    r = engine.exact_mixture(mean, var, info, [0, 3, 4, 5, 9])
    r8 = engine.exact_mixture(mean8, var8, info8, [0, 3, 4, 4, 8])
    assert r["kept"].cpu().tolist() == [3, 1, 0, 4] and r8["kept"].cpu().tolist() == [3, 1, 0, 4]
    assert bool(r["mean"][2].isnan().all()) and bool(r["var"][2].isnan().all())
    assert np.array_equal(bits(r["mean"][[0, 1, 3]], r["var"][[0, 1, 3]]), bits(r8["mean"][[0, 1, 3]], r8["var"][[0, 1, 3]]))
    one = engine.exact_mixture(mean, var, info, [0, 2, 9])  # draws 2..8 with the failed one among them: n - 1 of 7
    rest = engine.exact_mixture(mean8, var8, info8, [0, 2, 8])
    assert one["kept"].cpu().tolist() == [2, 6] and np.array_equal(bits(one["mean"], one["var"]), bits(rest["mean"], rest["var"]))
    m, v = mean8.cpu().numpy()[2:], var8.cpu().numpy()[2:]
    assert np.allclose(one["mean"][1].cpu().numpy(), m.mean(0), rtol=1e-13, atol=1e-15)
    assert np.allclose(one["var"][1].cpu().numpy(), (v + (m - m.mean(0)) ** 2).mean(0), rtol=1e-13)


def test_a_theta_that_is_not_positive_and_finite_is_reported(engine):
    rng = np.random.default_rng(4)
    X, y, Xs = rng.uniform(0, 10, (6, 2)), rng.standard_normal(6), rng.uniform(0, 10, (5, 2))
    th = bad_theta_rows()
    Xd, yd, Xsd = dev(X, engine), dev(y, engine), dev(Xs, engine)
    mean, var, info = engine.exact_predict_batch(Xd, yd, dev(th, engine), Xsd)
    assert info.cpu().tolist() == [0] + [1] * 7
    assert bool(mean[1:].isnan().all()) and bool(var[1:].isnan().all()) and bool(mean[0].isfinite().all())
    m1, v1, _ = engine.exact_predict_batch(Xd, yd, dev(th[:1], engine), Xsd)
    assert np.array_equal(bits(mean[:1], var[:1]), bits(m1, v1))
    r = engine.exact_mixture(mean, var, info, [0, 8])
    assert r["kept"].cpu().tolist() == [1] and np.array_equal(bits(r["mean"]), bits(m1))


# (f)
@pytest.mark.parametrize("N", [30, 120])
def test_batch_agrees_with_the_single_call_path(engine, N):
    rng = np.random.default_rng(N)
    d, T = 2, 40
    X = rng.uniform(0.0, 10.0, (N, d))
    y = 3.0 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 10.0, (T, d))
    th = np.array([[1.5, 2.5, 25.0, 1.0], [4.0, 3.0, 2.0, 0.1], [0.7, 0.9, 1.0, 0.3]])
    Xd, yd, Xsd = dev(X, engine), dev(y, engine), dev(Xs, engine)
    for pred_noise in (True, False):
        mean, var, info = engine.exact_predict_batch(Xd, yd, dev(th, engine), Xsd, pred_noise=pred_noise)
        mh, vh = mean.cpu().numpy(), var.cpu().numpy()
        assert int(info.abs().sum()) == 0
        for p in range(3):
            ls = list(th[p, :d])
            r = engine.exact_eval(Xd, yd, ls, th[p, d], th[p, d + 1], want_grad=False, want_factors=True)
            m1, v1, _ = engine.exact_predict(Xsd, Xd, ls, th[p, d], th[p, d + 1], r["factors"], pred_noise=pred_noise)
            ref = reference(X, y, Xs, th[p, :d], th[p, d], th[p, d + 1], pred_noise=pred_noise)
            assert r["info"] == 0
            lim_m = 2 * TAU * ref["cond"] * ref["S_mu"].astype(np.float64)
            lim_v = 2 * TAU * ref["cond"] * ref["S_v"].astype(np.float64)
            assert (np.abs(m1.cpu().numpy() - mh[p]) <= lim_m).all() and (np.abs(v1.cpu().numpy() - vh[p]) <= lim_v).all()


# (g)
def test_the_reduction_meets_its_derived_bounds(engine):
    check_mixture(engine, lambda a: dev(a, engine))


# (h)
def test_out_of_range_arguments_are_refused(engine):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=engine.device)  # noqa: E731
    for X, Y, th, Xs, kw, status in ((z(129, 1), z(129), z(2, 3), z(4, 1), {}, -2), (z(10, 9), z(10), z(2, 11), z(4, 9), {}, -2),
                                     (z(10, 2), z(10), z(2, 4), z(0, 2), {}, -1), (z(10, 2), z(10), z(2, 4), z(32769, 2), {}, -2),
                                     (z(10, 2), z(10), z(2, 4), z(4, 2), {"kernel": "composite"}, -1),
                                     (z(10, 2), z(10), z(0, 4), z(4, 2), {}, -1)):
        with pytest.raises(ggp_amd.SgpStatusError) as ei:
            engine.exact_predict_batch(X, Y, th, Xs, **kw)
        assert ei.value.status == status
    lib = engine.exact_predict_lib
    need = lib.sgp_exact_predict_batch_workspace_bytes(2, 10, 2, 5)
    assert need > 0 and lib.sgp_exact_predict_batch_workspace_bytes(2 ** 24, 10, 2, 5) == 0
    X, Y, Xs, th = z(10, 2), z(10), z(5, 2), torch.ones(2, 4, dtype=torch.float64, device=engine.device)
    mean, var = z(2, 5), z(2, 5)
    info = torch.zeros(2, dtype=torch.int32, device=engine.device)
    ws = torch.empty(need, dtype=torch.uint8, device=engine.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = lambda ws_ptr, nbytes, P=2, T=5, Xp=p(X): (Xp, 20, 2, p(Y), 10, p(Xs), 10, 2, T, None, None, None, p(th), P, 10, 2, 0, 1,  # noqa: E731
                                                      p(mean), p(var), p(info), ws_ptr, nbytes, engine._stream())
    assert lib.sgp_exact_predict_batch(*args(p(ws), need - 1)) == -3 and lib.sgp_exact_predict_batch(*args(None, need)) == -3
    assert lib.sgp_exact_predict_batch(*args(p(ws), need, P=2 ** 24)) == -2 and lib.sgp_exact_predict_batch(*args(p(ws), need, T=0)) == -1
    assert lib.sgp_exact_predict_batch(*args(p(ws), need, T=32769)) == -2 and lib.sgp_exact_predict_batch(*args(p(ws), need, Xp=None)) == -1
    torch.cuda.synchronize()
    assert float(mean.abs().sum()) == 0.0 and float(var.abs().sum()) == 0.0  # nothing was enqueued: the outputs are untouched
    assert lib.sgp_exact_predict_batch(*args(p(ws), need)) == 0
    torch.cuda.synchronize()
    assert bool(mean.isfinite().all()) and bool((var > 0).all()) and info.cpu().tolist() == [0, 0]
    # the mixture: offsets are checked on the host by the engine, everything else by the entry point
    for off in ([0, 1, 0, 2], [0, 1], [0, 3], [1, 2], []):
        with pytest.raises(ValueError):
            engine.exact_mixture(mean, var, info, off)
    mm, kept = z(1, 5), torch.zeros(1, dtype=torch.int32, device=engine.device)
    off = torch.as_tensor([0, 2], dtype=torch.int64, device=engine.device)
    mix = lambda G=1, T=5, nbytes=256, lp=None, y=None: lib.sgp_exact_mixture_reduce(  # noqa: E731
        p(mean), p(var), p(info), p(off), G, T, y, p(mm), p(mm), lp, None, p(kept), p(ws), nbytes, engine._stream())
    assert mix(G=0) == -1 and mix(T=32769) == -2 and mix(nbytes=255) == -3 and mix(y=p(mean)) == -1 and mix(G=2 ** 24) == -2
    torch.cuda.synchronize()
    assert float(mm.abs().sum()) == 0.0
    for k in range(3):
        small, middle, large = (lib.sgp_exact_predict_batch_occupancy(N, k) for N in (32, 64, 128))
        print("kernel %d: workgroups per CU %d / %d / %d" % (k, small, middle, large))
        assert small >= middle >= large >= 1
    assert lib.sgp_exact_predict_batch_occupancy(129, 0) == -2 and lib.sgp_exact_predict_batch_occupancy(10, 3) == -1


# (i)
def test_nuts_draws_to_predictions_end_to_end(engine):
    rng = np.random.default_rng(12)
    B, N, T = 3, 20, 15
    X = np.sort(rng.uniform(0.0, 10.0, (N, 1)), 0)
    Y = np.sin(X[:, 0])[None] * np.array([[1.0], [2.0], [0.5]]) + 0.2 * rng.standard_normal((B, N))
    Xt = rng.uniform(0.0, 10.0, (T, 1))
    Yt = np.sin(Xt[:, 0])[None] * np.array([[1.0], [2.0], [0.5]]) + 0.2 * rng.standard_normal((B, T))
    post = ggp_amd.sample_exact_nuts_batch(X, Y, 20, 50, chains=2, seed=3, engine=engine)
    r = post.predict(Xt, Yt, thin=2)
    S = 2 * 10
    assert r.draw_mean.shape == (B, S, T) and r.kept.tolist() == [S] * B and not r.info.any()
    q = post.samples[:, :, ::2].reshape(B * S, 3)
    th = np.concatenate([np.exp(q[:, :1]), np.exp(q[:, 1:]) ** 2], 1)
    th[:, 2] = np.where(th[:, 2] < 1e-4, 0.01 ** 2, th[:, 2])
    set_of = np.repeat(np.arange(B, dtype=np.int32), S)
    mean, var, info = engine.exact_predict_batch(dev(X, engine), dev(Y, engine), dev(th, engine), dev(Xt, engine), iy=set_of)
    assert np.array_equal(bits(mean), r.draw_mean.reshape(-1).view(np.uint64)) and np.array_equal(bits(var), r.draw_var.reshape(-1).view(np.uint64))
    l = -0.5 * np.log(2 * np.pi * r.draw_var) - 0.5 * (Yt[:, None] - r.draw_mean) ** 2 / r.draw_var
    c = (np.abs(0.5 * np.log(2 * np.pi * r.draw_var)) + 0.5 * (Yt[:, None] - r.draw_mean) ** 2 / r.draw_var).max(1)
    mx = l.max(1, keepdims=True)
    want = (mx[:, 0] + np.log(np.exp(l - mx).mean(1)))
    # the device's bound and as much again for this float64 formula
    assert (np.abs(r.logpdf - want) <= 2 * EPS * (8 * c + S + 8)).all()
    assert (np.abs(r.nlpd(2.0) - (-want.mean(1) + np.log(2.0))) <= 2 * EPS * (8 * c + S + 8).mean(1) + 4 * EPS * np.abs(want).mean(1)).all()
    assert np.isfinite(r.rmse(Yt)).all() and (r.rmse(Yt) < 1.0).all()
    fit = ggp_amd.fit_ml2(X, Y, theta0=[1.0, 1.0, 0.1], bounds=np.array([(1e-2, 1e3), (1e-5, 1e5), (1e-5, 1e5)]), n_restarts=2, seed=0,
                          engine=engine)
    p = fit.predict(Xt, Yt)
    assert p.draw_mean.shape == (B, 1, T) and p.kept.tolist() == [1] * B
    assert np.isfinite(p.mean).all() and np.isfinite(p.var).all() and np.isfinite(p.nlpd()).all() and np.isfinite(p.rmse(Yt)).all()
