"""GPU: sgp_mixture_quantiles (csrc/sgp_mixture.hip) under the acceptance rule of tests/mixture_quantile_reference.py on every family
at the edges of the 256-point chunk and for Q = 1, 2, 5, 8, every (group, test point) alone against its bits in the batch, a second
launch / stream / context, the degenerate inputs, agreement with the host interval function, the refusals of the C ABI, and
``predict(..., probs=...)`` end to end for the exact and the sparse sampler."""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_quantile_reference as R
from conftest import dev

import ggp_amd

pytestmark = pytest.mark.gpu
MORE = (0.1, 0.25, 0.9)   # with R.PROBS: Q = 8


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint64)


def idev(a, engine):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(engine.device)


def run(engine, mean, var, info, off, probs, Y=None, want_iters=False):
    r = engine.mixture_quantiles(dev(mean, engine), dev(var, engine), idev(info, engine), off, probs,
                                 Ytest=None if Y is None else dev(Y, engine), want_iters=want_iters)
    return r["quantiles"], r["pit"], r["iters"]


# 1
@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_families_and_shapes_meet_the_acceptance_rule(engine, T):
    mean, var, info, off, Y, names = R.batch(T)
    quant, pit, iters = run(engine, mean, var, info, off, R.PROBS, Y, want_iters=True)
    qh, ph, ih = quant.cpu().numpy(), pit.cpu().numpy(), iters.cpu().numpy()
    worst = R.check_batch(qh, ph, ih, R.PROBS, mean, var, info, off, Y, names)
    print("T=%d: worst %s; passes per family %s" % (T, worst, dict(zip(names, ih.max(1).tolist()))))
    assert ih[names.index("empty")].max() == 0
    # Q = 8, 2 and 1: other instantiations and other neighbours in the call, the same bits for a probability they share
    q8, p8, _ = run(engine, mean, var, info, off, R.PROBS + MORE, Y)
    assert np.array_equal(bits(q8[:, :5]), bits(quant)) and np.array_equal(bits(p8), bits(pit))
    R.check_batch(q8.cpu().numpy(), None, None, R.PROBS + MORE, mean, var, info, off, Y, names, columns=[T - 1])
    q2, _, _ = run(engine, mean, var, info, off, (0.975, 0.025))
    assert np.array_equal(bits(q2[:, 0]), bits(quant[:, 3])) and np.array_equal(bits(q2[:, 1]), bits(quant[:, 1]))
    q1, p1, _ = run(engine, mean, var, info, off, (1e-9,), Y)
    assert np.array_equal(bits(q1[:, 0]), bits(quant[:, 0])) and np.array_equal(bits(p1), bits(pit))
    if T == 1:   # S = 1, mu = 3, sigma = 2: mu + sigma Phi^-1(p)
        g = names.index("single")
        assert abs(qh[g, 3, 0] - (3.0 + 2.0 * 1.959963984540054)) < 1e-13 and abs(qh[g, 2, 0] - 3.0) < 1e-13


# 2
def test_every_point_alone_has_its_bits_of_the_batch_on_every_launch_stream_and_context(engine):
    T = 257
    mean, var, info, off, Y, names = R.batch(T)
    md, vd, idv, Yd = dev(mean, engine), dev(var, engine), idev(info, engine), dev(Y, engine)
    whole = engine.mixture_quantiles(md, vd, idv, off, R.PROBS, Ytest=Yd)
    wq, wp = bits(whole["quantiles"]), bits(whole["pit"])
    for g, name in enumerate(names):
        s0, s1 = int(off[g]), int(off[g + 1])
        for t in (0, 1, 2, 255, 256):
            if name == "empty":
                continue
            one = engine.mixture_quantiles(md[s0:s1, t:t + 1].contiguous(), vd[s0:s1, t:t + 1].contiguous(), idv[s0:s1].contiguous(),
                                           [0, s1 - s0], R.PROBS, Ytest=Yd[g:g + 1, t:t + 1].contiguous())
            assert np.array_equal(bits(one["quantiles"])[0, :, 0], wq[g, :, t]), (name, t)
            assert bits(one["pit"])[0, 0] == wp[g, t], (name, t)
    # the groups in another order and other company: the same bits
    order = [5, 0, 3]
    rows = np.concatenate([np.arange(off[g], off[g + 1]) for g in order])
    off2 = np.concatenate([[0], np.cumsum([off[g + 1] - off[g] for g in order])])
    moved = engine.mixture_quantiles(dev(mean[rows], engine), dev(var[rows], engine), idev(info[rows], engine), off2, R.PROBS,
                                     Ytest=dev(Y[order], engine))
    assert np.array_equal(bits(moved["quantiles"]), wq[order]) and np.array_equal(bits(moved["pit"]), wp[order])
    # a second launch, a second stream, a context of its own
    again = engine.mixture_quantiles(md, vd, idv, off, R.PROBS, Ytest=Yd)
    assert np.array_equal(bits(again["quantiles"]), wq) and np.array_equal(bits(again["pit"]), wp)
    other = ggp_amd.HipEngine(own_context=True)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        r = other.mixture_quantiles(md, vd, idv, off, R.PROBS, Ytest=Yd)
    stream.synchronize()
    assert np.array_equal(bits(r["quantiles"]), wq) and np.array_equal(bits(r["pit"]), wp)


# 3
def test_degenerate_inputs_stay_local(engine):
    T = 5
    mean, var, info, off, Y, names = R.batch(T)
    base_q, base_p, _ = run(engine, mean, var, info, off, R.PROBS, Y)
    gm, gs, gi = names.index("many"), names.index("scales"), names.index("identical")
    m1, v1 = mean.copy(), var.copy()
    v1[off[gm] + 5, 1] = 0.0
    v1[off[gm] + 999, 2] = -1.0
    m1[off[gs], 3] = np.nan
    v1[off[gs] + 63, 4] = np.nan
    v1[off[gi] + 1, 0] = np.inf
    q1, p1, it1 = run(engine, m1, v1, info, off, R.PROBS, Y, want_iters=True)
    hit = np.zeros((len(names), T), dtype=bool)
    hit[gm, 1] = hit[gm, 2] = hit[gs, 3] = hit[gs, 4] = hit[gi, 0] = True
    hit[names.index("empty")] = True
    q1h, p1h = q1.cpu().numpy().transpose(0, 2, 1), p1.cpu().numpy()
    assert np.isnan(q1h[hit]).all() and np.isnan(p1h[hit]).all() and (it1.cpu().numpy()[hit] == 0).all()
    keep = ~hit
    assert np.array_equal(q1h[keep].view(np.uint64), base_q.cpu().numpy().transpose(0, 2, 1)[keep].view(np.uint64))
    assert np.array_equal(p1h[keep].view(np.uint64), base_p.cpu().numpy()[keep].view(np.uint64))
    # a failed draw's NaN row is never read: the masked group is the group without those draws
    gk = names.index("masked")
    rows = np.arange(off[gk], off[gk + 1])[info[off[gk]:off[gk + 1]] == 0]
    alone, _, _ = run(engine, mean[rows], var[rows], info[rows], [0, rows.size], R.PROBS)
    assert np.array_equal(bits(alone)[0], bits(base_q)[gk])
    # without Ytest, pit is not written (and may be NULL); iters is optional
    lib = engine.mixture_lib
    md, vd, idv = dev(mean, engine), dev(var, engine), idev(info, engine)
    offd = torch.as_tensor(off).to(engine.device)
    G = len(names)
    quant = torch.zeros(G, 2, T, dtype=torch.float64, device=engine.device)
    pit = torch.full((G, T), 7.0, dtype=torch.float64, device=engine.device)
    ws = torch.empty(256, dtype=torch.uint8, device=engine.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pr = (C.c_double * 2)(0.025, 0.975)
    assert lib.sgp_mixture_quantiles(p(md), p(vd), p(idv), p(offd), G, T, pr, 2, None, p(quant), p(pit), None, p(ws), 256,
                                     engine._stream()) == 0
    assert lib.sgp_mixture_quantiles(p(md), p(vd), p(idv), p(offd), G, T, pr, 2, None, p(quant), None, None, p(ws), 256,
                                     engine._stream()) == 0
    torch.cuda.synchronize()
    assert bool((pit == 7.0).all()) and np.array_equal(bits(quant), bits(base_q[:, [1, 3]]))


# 4
@pytest.mark.parametrize("name", ["many", "scales"])
def test_agreement_with_the_host_interval_function(engine, name):
    """|x_dev - x_host| <= W + 2 e / f_ref(x): both answers solve the same equation, each to a tail error of at most e."""
    mu, sg = R.family(name, 0)
    quant, _, _ = run(engine, mu[:, None], (sg * sg)[:, None], np.zeros(mu.size, dtype=np.int32), [0, mu.size], (0.025, 0.975))
    lo, hi = ggp_amd.get_posterior_predictive_uncertainty_intervals(mu[:, None], np.sqrt(sg * sg)[:, None])
    sgk = np.sqrt(sg * sg)
    for x, host, p in ((float(quant[0, 0, 0]), float(lo[0]), 0.025), (float(quant[0, 1, 0]), float(hi[0]), 0.975)):
        e = R.mq_err(mu.size, R.split(p)[0], R.sens_ref(x, mu, sgk))
        allowed = R.width(x, float(sgk.min())) + 2.0 * e / R.dens_ref(x, mu, sgk)
        print("%s p=%g: device %.17g host %.17g |diff| %.3e allowed %.3e" % (name, p, x, host, abs(x - host), allowed))
        assert abs(x - host) <= allowed, (name, p, x, host, allowed)


# 5
def test_out_of_range_arguments_are_refused(engine):
    lib = engine.mixture_lib
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=engine.device)  # noqa: E731
    mean, var, info = z(4, 5), torch.ones(4, 5, dtype=torch.float64, device=engine.device), torch.zeros(4, dtype=torch.int32,
                                                                                                       device=engine.device)
    off = torch.as_tensor([0, 1, 4], dtype=torch.int64, device=engine.device)
    quant, pit = z(2, 2, 5), z(2, 5)
    ws = torch.empty(256, dtype=torch.uint8, device=engine.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(fn=lib.sgp_mixture_quantiles, ctx=(), probs=(0.025, 0.975), Q=None, G=2, T=5, m=mean, o=off, qt=quant, y=None, pt=pit, w=ws,
             nbytes=256):
        pr = None if probs is None else (C.c_double * len(probs))(*probs)
        return fn(*ctx, p(m), p(var), p(info), p(o), G, T, pr, len(probs) if Q is None else Q, p(y), p(qt), p(pt), None, p(w), nbytes,
                  engine._stream())
    nine = tuple(0.1 * k for k in range(1, 10))
    for kw, want in ((dict(m=None), -1), (dict(o=None), -1), (dict(qt=None), -1), (dict(probs=None, Q=1), -1), (dict(y=mean, pt=None), -1),
                     (dict(Q=0), -1), (dict(probs=nine), -1), (dict(probs=(0.5, 1e-10)), -1), (dict(probs=(1.0,)), -1),
                     (dict(probs=(float("nan"),)), -1), (dict(G=0), -1), (dict(T=0), -1), (dict(G=2 ** 24), -2), (dict(T=32769), -2),
                     (dict(w=None), -3), (dict(nbytes=255), -3), (dict(G=2 ** 24, probs=(2.0,)), -1), (dict(T=32769, nbytes=0), -2)):
        assert call(**kw) == want, kw
        assert call(fn=lib.sgp_ctx_mixture_quantiles, ctx=(None,), **kw) == want, kw
    torch.cuda.synchronize()
    assert float(quant.abs().sum()) == 0.0   # nothing was enqueued
    assert call() == 0 and call(fn=lib.sgp_ctx_mixture_quantiles, ctx=(engine._c(),)) == 0
    torch.cuda.synchronize()
    assert bool(quant.isfinite().all())
    for bad in (dict(probs=()), dict(probs=nine), dict(probs=(0.5, 2.0)), dict(offsets=[0, 1, 0, 4]), dict(offsets=[0, 3]), dict(offsets=[]),
                dict(info=info.long()), dict(mean=mean.float()), dict(Ytest=z(2, 4))):
        kw = dict(mean=mean, var=var, info=info, offsets=[0, 1, 4], probs=(0.5,))
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.mixture_quantiles(**kw)


# 6
def _unimodal(mu, sd, lower, upper):
    x = np.linspace(lower - (upper - lower), upper + (upper - lower), 801)
    f = (np.exp(-0.5 * ((x[:, None] - mu[None]) / sd[None]) ** 2) / sd[None]).sum(1)
    return int(((f[1:-1] > f[:-2]) & (f[1:-1] >= f[2:])).sum()) == 1


def test_nuts_draws_to_intervals_end_to_end(engine):
    rng = np.random.default_rng(21)
    B, N, M, T = 2, 24, 8, 16
    X = np.sort(rng.uniform(0.0, 10.0, (N, 1)), 0)
    Y = np.sin(X[:, 0])[None] * np.array([[1.0], [2.0]]) + 0.2 * rng.standard_normal((B, N))
    Xt = rng.uniform(0.0, 10.0, (T, 1))
    Yt = np.sin(Xt[:, 0])[None] * np.array([[1.0], [2.0]]) + 0.2 * rng.standard_normal((B, T))
    Z = X[np.round(np.linspace(0, N - 1, M)).astype(int)].copy()
    probs = (0.025, 0.5, 0.975)
    posts = (ggp_amd.sample_exact_nuts_batch(X, Y, 20, 20, chains=2, seed=3, engine=engine),
             ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 20, 20, chains=2, seed=3, engine=engine))
    for post in posts:
        plain = post.predict(Xt, Yt)
        r = post.predict(Xt, Yt, probs=probs)
        assert plain.quantiles is None and plain.pit is None and plain.probs is None
        assert np.array_equal(r.mean, plain.mean) and np.array_equal(r.logpdf, plain.logpdf)
        assert r.probs.tolist() == list(probs) and r.quantiles.shape == (B, 3, T) and r.pit.shape == (B, T)
        assert np.isfinite(r.quantiles).all() and ((r.pit > 0) & (r.pit < 1)).all() and (np.diff(r.quantiles, axis=1) > 0).all()
        lower, upper = r.interval(0.95)
        checked = 0
        for b in range(B):
            keep = r.info[b] == 0
            for t in range(T):
                mu, sd = r.draw_mean[b, keep, t], np.sqrt(r.draw_var[b, keep, t])
                for q, p in enumerate(probs):   # the acceptance rule on the draws' own moments
                    ok, fig = R.accept(float(r.quantiles[b, q, t]), p, mu, sd)
                    assert ok, (b, t, fig)
                assert abs(r.pit[b, t] - R.pit_ref(float(Yt[b, t]), mu, sd)) <= R.pit_bound(mu.size)
                if _unimodal(mu, sd, lower[b, t], upper[b, t]):
                    assert lower[b, t] < r.mean[b, t] < upper[b, t]
                    checked += 1
        assert checked > B * T // 2
        assert np.array_equal(r.coverage(0.95), ((Yt >= lower) & (Yt <= upper)).mean(1))
        assert np.array_equal(r.interval_width(0.95), (upper - lower).mean(1)) and (r.interval_width(0.95) > 0).all()
        # the host-moments route gives the bits of the device-resident one
        quant, pit = ggp_amd.mixture_quantiles(r.draw_mean, r.draw_var, probs, info=r.info, y=Yt, engine=engine)
        assert np.array_equal(quant.view(np.uint64), r.quantiles.view(np.uint64)) and np.array_equal(pit.view(np.uint64), r.pit.view(np.uint64))
