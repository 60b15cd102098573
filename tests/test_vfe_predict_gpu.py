"""GPU: sgp_vfe_predict_batch (csrc/sgp_vfe_predict.hip, one workgroup per problem) against the long-double reference
tests/vfe_predict_reference.py at the cells of the three size classes and across the test tile of each, ``bound`` against
sgp_vfe_eval_batch bit for bit, the batch plumbing bit for bit (streams and contexts included), the failure paths, the agreement with
the single-data-set route ``mixture_predict``, the occupancy query, and ``SgprNutsResult.predict`` / ``SgprBatchResult.predict`` end to
end.  The checks themselves are those of tests/test_vfe_predict.py, run there on the CPU double."""
import numpy as np
import pytest
import torch

import vfe_batch_double as VB
import vfe_predict_reference as R
from conftest import dev
from test_vfe_batch_gpu import fit_data
from test_vfe_predict import (T_EDGE_CELLS, check_bound_is_the_batched_bound, check_cell, check_failures_stay_local, check_mixture_of_draws,
                              check_t_edges, np64, same_bits)

import ggp_amd

pytestmark = pytest.mark.gpu
POISON = -7.25   # what the outputs hold before a launch


# (a)
@pytest.mark.parametrize("name", R.CELLS)
def test_cells_match_the_long_double_reference(engine, name):
    worst = check_cell(engine, lambda a: dev(a, engine), name)
    print("VFE_PREDICT %s: worst error / tolerance: mean %.3g, var %.3g" % (name, worst["mean"], worst["var"]))


# (b)
@pytest.mark.parametrize("name", T_EDGE_CELLS)
def test_t_edges_meet_the_bound_with_the_bits_of_the_long_call(engine, name):
    check_t_edges(engine, lambda a: dev(a, engine), name, bits=True)


# (c)
def test_bound_has_the_bits_of_the_batched_bound(engine):
    check_bound_is_the_batched_bound(engine, lambda a: dev(a, engine))


# (d)
def batch_problem(P, seed=5, T=37):
    """P problems over 3 data sets x 2 targets x 3 inducing sets x 2 test sets at (N, M, d) = (65, 17, 2); T = 37: not a multiple of the
    middle class's tile of 64."""
    rng = np.random.default_rng(seed)
    N, M, d = 65, 17, 2
    X = rng.standard_normal((3, N, d))
    Y = np.stack([np.sin(X[0].sum(1)), np.cos(X[1, :, 0])]) + 0.1 * rng.standard_normal((2, N))
    Z = np.stack([X[s][rng.permutation(N)[:M]] for s in range(3)])
    Xs = 1.5 * rng.standard_normal((2, T, d))
    theta = np.exp(np.concatenate([rng.uniform(np.log(0.6), np.log(1.6), (P, d)), rng.uniform(np.log(0.5), np.log(2.0), (P, 1)),
                                   rng.uniform(np.log(0.03), np.log(0.3), (P, 1))], 1))
    idx = [rng.integers(0, n, P).astype(np.int32) for n in (3, 2, 3, 2)]
    return X, Y, Z, Xs, theta, idx


def raw_launch(engine, ctx, Xd, Yd, Zd, Xsd, thd, idx, T, kernel_id, pad=96):
    """The C entry point (``ctx``: the context twin) on poisoned outputs with ``pad`` doubles after the P x T the kernel may write."""
    P, (N, d), M = thd.shape[0], Xd.shape[1:], Zd.shape[1]
    mean, var = engine.empty(P * T + pad).fill_(POISON), engine.empty(P * T + pad).fill_(POISON)
    bound = engine.empty(P + pad).fill_(POISON)
    info = torch.full((P + pad,), -99, dtype=torch.int32, device=engine.device)
    ws = engine._workspace("vfe_predict", 256)
    ws.fill_(0xFF)
    ixd, iyd, izd, ixsd = (torch.as_tensor(a, device=engine.device) for a in idx)
    p_ = engine._ptr
    args = (p_(Xd), N * d, d, p_(Yd), N, p_(ixd), p_(iyd), p_(Zd), M * d, d, p_(izd), p_(Xsd), Xsd.shape[1] * d, d, T, p_(ixsd), p_(thd), P, N,
            M, d, kernel_id, 1e-6, 1, p_(mean), p_(var), p_(bound), p_(info), p_(ws), ws.numel(), engine._stream())
    lib = engine.vfe_predict_lib
    assert (lib.sgp_ctx_vfe_predict_batch(engine._c(), *args) if ctx else lib.sgp_vfe_predict_batch(*args)) == 0
    torch.cuda.synchronize()
    return mean, var, bound, info


@pytest.mark.parametrize("P", [1, 2, 600])
def test_every_problem_of_a_batch_equals_the_problem_alone(engine, P):
    X, Y, Z, Xs, theta, idx = batch_problem(P)
    ix, iy, iz, ixs = idx
    T = Xs.shape[1]
    Xd, Yd, Zd, Xsd, thd = (dev(a, engine) for a in (X, Y, Z, Xs, theta))
    kw = dict(ix=ix, iy=iy, iz=iz, ixs=ixs, kernel="matern52", jitter=1e-6)
    mean, var, bound, info = engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, **kw)
    assert int(info.abs().sum()) == 0 and bool(mean.isfinite().all()) and bool(var.isfinite().all())
    alone = [engine.vfe_predict_batch(Xd[ix[p]].contiguous(), Yd[iy[p]].contiguous(), Zd[iz[p]].contiguous(), thd[p:p + 1].contiguous(),
                                      Xsd[ixs[p]].contiguous(), kernel="matern52", jitter=1e-6) for p in range(P)]
    assert same_bits(torch.cat([a[0] for a in alone]), mean) and same_bits(torch.cat([a[1] for a in alone]), var)
    assert same_bits(torch.cat([a[2] for a in alone]), bound) and int(torch.cat([a[3] for a in alone]).abs().sum()) == 0
    # the plain entry point and the context twin on poisoned outputs: the same bits, and nothing past P x T, P is written
    for ctx in (False, True):
        m, v, b, i = raw_launch(engine, ctx, Xd, Yd, Zd, Xsd, thd, idx, T, 2)
        assert same_bits(m[:P * T].reshape(P, T), mean) and same_bits(v[:P * T].reshape(P, T), var) and same_bits(b[:P], bound)
        assert bool((m[P * T:] == POISON).all()) and bool((v[P * T:] == POISON).all()) and bool((b[P:] == POISON).all())
        assert i[:P].tolist() == [0] * P and bool((i[P:] == -99).all())
    # a shorter T on the same test sets (their stride stays): rows of T - 5 points, the rest of the buffer untouched
    m, v, _, _ = raw_launch(engine, False, Xd, Yd, Zd, Xsd, thd, idx, T - 5, 2)
    assert same_bits(m[:P * (T - 5)].reshape(P, T - 5), mean[:, :T - 5]) and same_bits(v[:P * (T - 5)].reshape(P, T - 5), var[:, :T - 5])
    assert bool((m[P * (T - 5):] == POISON).all()) and bool((v[P * (T - 5):] == POISON).all())
    for bad in ({"ix": [3] * P}, {"iy": [5] * P}, {"iz": [3] * P}, {"ixs": [2] * P}, {"ixs": [-1] * P}):
        with pytest.raises(ValueError):
            engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, **{**kw, **bad})


def test_same_bits_on_a_second_stream_and_a_context_of_its_own(engine):
    X, Y, Z, Xs, theta, idx = batch_problem(64, seed=6)
    ix, iy, iz, ixs = idx
    Xd, Yd, Zd, Xsd, thd = (dev(a, engine) for a in (X, Y, Z, Xs, theta))
    kw = dict(ix=ix, iy=iy, iz=iz, ixs=ixs, kernel="rbf", jitter=1e-6)
    first = engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, **kw)
    again = engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, **kw)
    assert all(same_bits(a, b) for a, b in zip(first[:3], again[:3]))
    own = ggp_amd.HipEngine(own_context=True)
    side = torch.cuda.Stream(device=engine.device)
    side.wait_stream(torch.cuda.current_stream(engine.device))
    with torch.cuda.stream(side):
        s_eng = engine.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, **kw)
        s_own = own.vfe_predict_batch(Xd, Yd, Zd, thd, Xsd, **kw)
    side.synchronize()
    for other in (s_eng, s_own):
        assert all(same_bits(a, b) for a, b in zip(first[:3], other[:3])) and int(other[3].abs().sum()) == 0


# (e)
def test_failures_stay_local(engine):
    check_failures_stay_local(engine, lambda a: dev(a, engine))


# (f)
@pytest.mark.parametrize("name", ["65-17-2-rbf", "200-64-2-matern32"])
def test_agreement_with_the_single_data_set_route(engine, name):
    """``mixture_predict(full_cov=False)`` and the batched kernel at 8 draws around the cell's theta: each within its own tolerance of
    the long-double reference (the two differ in op order: bits are not compared)."""
    import vfe_reference as V
    inp = VB.inputs(name)
    d = VB.spec(name)["d"]
    Xs = R.cell_points(name)
    rng = np.random.default_rng(8)
    theta = inp["theta"][None] * np.exp(rng.uniform(-0.2, 0.2, (8, d + 2)))
    X, y, Z, Xsd = (dev(a, engine) for a in (inp["X"], inp["y"], inp["Z"], Xs))
    mean, var, _, info = engine.vfe_predict_batch(X, y, Z, dev(theta, engine), Xsd, kernel=inp["kernel"], jitter=inp["jitter"])
    old = engine.mixture_predict(X, y, Xsd, Z, theta[:, :d].tolist(), theta[:, d].tolist(), theta[:, d + 1].tolist(), jitter=inp["jitter"],
                                 kernel=inp["kernel"], pred_noise=True, full_cov=False)
    assert int(info.abs().sum()) == 0 and int(old["info"].abs().sum()) == 0
    for s in range(8):
        args = (inp["X"], inp["y"], inp["Z"], Xs, theta[s, :d], theta[s, d], theta[s, d + 1], inp["jitter"], inp["kernel"])
        ref, S = R.predictive(*args)
        e = {k: 0.0 for k in R.KEYS}
        for order in ("inverse", "substitution"):
            w = R.worst(R.predictive(*args, True, np.float64, order)[0], ref, S)
            e = {k: max(e[k], w[k]) for k in R.KEYS}
        for what, m, v in (("batched", mean, var), ("mixture_predict", old["mean"], old["var"])):
            w = R.worst({"mean": np64(m)[s], "var": np64(v)[s]}, ref, S)
            print("VFE_PREDICT %s draw %d %s: mean %.2g/%.1e var %.2g/%.1e" % (name, s, what, w["mean"], V.tolerance(e["mean"]), w["var"],
                                                                              V.tolerance(e["var"])))
            assert all(w[k] <= V.tolerance(e[k]) for k in R.KEYS), (what, s, w, e)


# (g)
def test_occupancy_query(engine):
    occ = engine.vfe_predict_lib.sgp_vfe_predict_batch_occupancy
    for kid in (0, 1, 2):
        small, middle, large = occ(16, kid), occ(32, kid), occ(64, kid)
        print("VFE_PREDICT occupancy kernel %d: %d / %d / %d workgroups per CU" % (kid, small, middle, large))
        assert small >= middle >= large >= 1
        assert occ(1, kid) == small and occ(17, kid) == middle and occ(33, kid) == large


# (h)
def test_nuts_draws_to_predictions_end_to_end(engine):
    X, Y, Z = fit_data()   # B = 3, N = 60, M = 8
    rng = np.random.default_rng(4)
    Xt = np.sort(rng.uniform(-3.0, 3.0, (3, 25, 1)), 1)
    Yt = np.sin(2.0 * Xt[:, :, 0]) * np.array([1.0, 0.5, 2.0])[:, None] + 0.2 * rng.standard_normal((3, 25))
    post = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 30, 30, chains=2, seed=7, engine=engine)
    r = post.predict(Xt, Yt)
    assert isinstance(r, ggp_amd.SgprMixturePredictive) and r.draw_mean.shape == (3, 60, 25) and r.kept.tolist() == [60] * 3
    for a in (r.mean, r.var, r.draw_mean, r.draw_var, r.bound, r.logpdf, r.mean_logpdf, r.nlpd(), r.rmse(Yt)):
        assert np.isfinite(a).all()
    assert (r.var > 0).all() and (r.info == 0).all()
    print("VFE_PREDICT end to end: nlpd %s rmse %s, mixture error / bound %s" % (r.nlpd(), r.rmse(Yt), check_mixture_of_draws(r, Yt)))
    thin = post.predict(Xt, thin=3)
    assert thin.draw_mean.shape == (3, 20, 25) and thin.logpdf is None
    assert np.array_equal(thin.draw_mean, r.draw_mean.reshape(3, 2, 30, 25)[:, :, ::3].reshape(3, 20, 25))
    # the plug-in predictive of a fit is the theta-row predictive at the fitted theta and Z
    fit = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=10, lr=0.05, seed=3, engine=engine)
    p = fit.predict(Xt, Yt)
    want = ggp_amd.sgpr_predict.predict_sgpr_theta_batch(X, Y, fit.Z, fit.theta[:, None, :], Xt, Yt, kernel=fit.kernel, jitter=fit.jitter,
                                                         engine=engine)
    assert p.draw_mean.shape == (3, 1, 25) and p.kept.tolist() == [1, 1, 1] and np.isfinite(p.nlpd()).all()
    assert np.array_equal(p.mean, want.mean) and np.array_equal(p.var, want.var) and np.array_equal(p.bound, want.bound)
    assert np.array_equal(p.mean, p.draw_mean[:, 0])
