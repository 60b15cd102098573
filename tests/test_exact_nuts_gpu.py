"""GPU: the batched device-resident NUTS over the exact GP (csrc/sgp_exact_nuts.hip) -- the device chain against the host-driven one
at the edges of the three size classes, its logp column against the batched evaluation, and that nothing but the per-draw seconds
depends on how the run is cut into launches, on what else shares the batch, on the call, the stream or the context; bad starts,
divergences, the posterior pin, occupancy and refusals, and GPR_HMC(device_sampler=True) end to end.

The DESIGN 6e-3 resource table this file asserts: chains per CU 2 / 2 / 1 for N <= 32 / <= 64 / <= 128."""
import numpy as np
import pytest
import torch

from conftest import dev
from exact_double import ExactDouble
from exact_nuts_double import ExactNutsDouble
from test_exact_nuts import T, pin_run

import ggp_amd
import ggp_amd._lib as L
from ggp_amd.exact_nuts import logp_batch

pytestmark = pytest.mark.gpu

CELLS = [(1, 1, "rbf"), (17, 1, "rbf"), (32, 2, "matern32"), (33, 8, "matern52"), (64, 3, "rbf"), (65, 2, "matern32"), (128, 8, "rbf")]
TUNE, DRAWS, DEPTH = 20, 15, 8
KEYS = ("samples", "stats", "evaluations", "draws", "info")


def bits(r, rows=slice(None)):
    """Everything a run returns but the per-draw seconds, as integers."""
    return np.concatenate([np.ascontiguousarray(np.asarray(r[k])[rows]).reshape(-1).view(
        {8: np.uint64, 4: np.uint32}[np.asarray(r[k]).dtype.itemsize]).astype(np.uint64) for k in KEYS])


def problem(N, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3.0, 3.0, (N, d))
    y = np.sin(X.sum(1)) + 0.2 * rng.standard_normal(N)
    q0 = np.array([np.log(2.0)] * d + [0.0, 0.0]) + rng.uniform(-0.3, 0.3, d + 2)
    return X, y, q0


_RUNS = {}


def cell_run(engine, cell):
    """The device chain of a cell (computed once, shared by the tests below, never modified)."""
    if cell not in _RUNS:
        N, d, kernel = cell
        X, y, q0 = problem(N, d, 100 * N + d)
        seed = 4000 + N
        Xd, yd = dev(X, engine), dev(y, engine)
        r = engine.exact_nuts_batch(Xd, yd, q0[None], [seed], TUNE, DRAWS, kernel=kernel, max_treedepth=DEPTH)
        _RUNS[cell] = (Xd, yd, q0, seed, r)
    return _RUNS[cell]


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "N%d-d%d-%s" % c)
def test_device_chain_is_the_host_driven_chain(engine, cell):
    """hmc.NUTS(rng=SplitMix(seed)) over engine.exact_eval_batch (P = 1) + theta_logp_and_grad from the same q0: identical trees, draws
    equal to rounding (the tolerances of tests/test_small.py for the sparse sampler)."""
    N, d, kernel = cell
    Xd, yd, q0, seed, r = cell_run(engine, cell)
    assert int(r["info"][0]) == 0 and int(r["draws"][0]) == TUNE + DRAWS
    h = ExactNutsDouble(evaluator=engine).exact_nuts_batch(Xd, yd, q0[None], [seed], TUNE, DRAWS, kernel=kernel, max_treedepth=DEPTH)
    assert int(h["info"][0]) == 0
    print("N=%d d=%d %s: %d evaluations, tree sizes %s" % (N, d, kernel, int(r["evaluations"][0]), r["stats"][0, :, 1].tolist()))
    assert int(r["evaluations"][0]) == int(h["evaluations"][0])
    assert np.array_equal(r["stats"][0, :, 1].numpy(), h["stats"][0, :, 1].numpy())
    assert np.allclose(r["stats"][0, :, 0].numpy(), h["stats"][0, :, 0].numpy(), rtol=1e-9, atol=0.0)
    assert np.allclose(r["samples"][0].numpy(), h["samples"][0].numpy(), rtol=1e-7, atol=1e-9)
    assert np.array_equal(r["stats"][0, :, 7].numpy(), h["stats"][0, :, 7].numpy()) and np.all(r["seconds"].numpy() > 0.0)


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "N%d-d%d-%s" % c)
def test_logp_column_is_the_batched_evaluation_at_the_draw(engine, cell):
    """exact_eval_batch at exp(sample) + prior + Jacobian, within 1e-10 (|logp| + N): the bound of test_gpr_hmc_gpu.check_against (the
    device's exp is within an ulp of libm's, hence no bit equality)."""
    N, d, kernel = cell
    Xd, yd, _, _, r = cell_run(engine, cell)
    lp = r["stats"][0, :, 6].numpy()
    ref, _ = logp_batch(engine, Xd, yd, r["samples"][0].numpy(), None, None, kernel)
    print("N=%d d=%d %s: max |logp - ref| / (|ref| + N) = %.3g" % (N, d, kernel, np.max(np.abs(lp - ref) / (np.abs(ref) + N))))
    assert np.isfinite(ref).all() and np.all(np.abs(lp - ref) <= 1e-10 * (np.abs(ref) + N))


@pytest.mark.parametrize("cell", [(33, 8, "matern52"), (128, 8, "rbf")], ids=lambda c: "N%d-d%d-%s" % c)
def test_the_result_does_not_depend_on_evals_per_launch(engine, cell):
    N, d, kernel = cell
    Xd, yd, q0, seed, r = cell_run(engine, cell)   # the default
    launches = [r["launches"]]
    for epl in (1, 5):
        c = engine.exact_nuts_batch(Xd, yd, q0[None], [seed], TUNE, DRAWS, kernel=kernel, max_treedepth=DEPTH, evals_per_launch=epl)
        assert np.array_equal(bits(c), bits(r)), epl
        launches.append(c["launches"])
    evals = int(r["evaluations"][0])
    print("N=%d: %d evaluations in %s launches (default, 1, 5 per launch)" % (N, evals, launches))
    assert launches[1] >= evals and evals / 5 <= launches[2] < launches[1]


def batch_problem():
    rng = np.random.default_rng(77)
    N, d, nX, nY, C = 30, 2, 7, 5, 600
    X = rng.uniform(-3.0, 3.0, (nX, N, d))
    Y = np.sin(X.sum(2))[rng.integers(0, nX, nY)] + 0.3 * rng.standard_normal((nY, N))
    ix, iy = rng.integers(0, nX, C).astype(np.int32), rng.integers(0, nY, C).astype(np.int32)
    q0 = np.array([np.log(2.0)] * d + [0.0, 0.0]) + rng.uniform(-0.5, 0.5, (C, d + 2))
    seeds = [int(s) for s in rng.integers(1, 2 ** 62, C)]
    return X, Y, ix, iy, q0, seeds


def test_a_chain_of_a_batch_is_the_chain_alone_on_every_call_stream_and_context(engine):
    """600 chains -- more than the chip holds at once -- over 7 data sets x 5 targets with scrambled ix / iy."""
    X, Y, ix, iy, q0, seeds = batch_problem()
    Xd, Yd = dev(X, engine), dev(Y, engine)
    kw = dict(kernel="matern32", max_treedepth=6)
    r = engine.exact_nuts_batch(Xd, Yd, q0, seeds, 10, 8, ix=ix, iy=iy, **kw)
    assert (r["info"] == 0).all() and (r["draws"] == 18).all() and np.isfinite(r["samples"].numpy()).all()
    for c in (0, 299, 599):
        one = engine.exact_nuts_batch(Xd[ix[c]].contiguous(), Yd[iy[c]].contiguous(), q0[c:c + 1], seeds[c:c + 1], 10, 8, **kw)
        assert np.array_equal(bits(one), bits(r, slice(c, c + 1))), c
    whole = bits(r)
    assert np.array_equal(bits(engine.exact_nuts_batch(Xd, Yd, q0, seeds, 10, 8, ix=ix, iy=iy, **kw)), whole)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        again = engine.exact_nuts_batch(Xd, Yd, q0, seeds, 10, 8, ix=ix, iy=iy, **kw)
    stream.synchronize()
    assert np.array_equal(bits(again), whole)
    other = ggp_amd.HipEngine(own_context=True)
    assert np.array_equal(bits(other.exact_nuts_batch(Xd, Yd, q0, seeds, 10, 8, ix=ix, iy=iy, evals_per_launch=7, **kw)), whole)


def test_bad_starts_are_reported_and_touch_nothing_else(engine):
    X, y, q = problem(20, 2, 5)
    Xd, yd = dev(X, engine), dev(y, engine)
    rng = np.random.default_rng(8)
    q0 = q + rng.uniform(-0.2, 0.2, (8, 4))
    q0[2, 1] = float("nan")
    q0[5, 3] = -301.0
    seeds = list(range(50, 58))
    r = engine.exact_nuts_batch(Xd, yd, q0, seeds, 10, 6, max_treedepth=6)
    bad = np.zeros(8, dtype=bool)
    bad[[2, 5]] = True
    assert np.array_equal(r["info"].numpy(), np.where(bad, L.EXACT_NUTS_BAD_START, 0))
    for k in ("samples", "stats", "seconds"):
        assert np.isnan(r[k].numpy()[bad]).all() and np.isfinite(r[k].numpy()[~bad]).all(), k
    assert (r["draws"].numpy()[bad] == 0).all() and (r["evaluations"].numpy()[bad] == 1).all() and (r["draws"].numpy()[~bad] == 16).all()
    six = engine.exact_nuts_batch(Xd, yd, q0[~bad], [s for s, b in zip(seeds, bad) if not b], 10, 6, max_treedepth=6)
    assert np.array_equal(bits(six), bits(r, ~bad))


def test_failed_factorisations_are_divergences_not_errors(engine):
    """Duplicated rows make A singular but for the noise.  The start at log sig_n = -40 has a finite density because sig_f (and y) are as
    small; the duplicates' share of log|A| then pulls sig_n down until sig_n^2 / sig_f^2 meets the pivot gate, and from there on the
    trajectories run into positions where the factorisation fails.  Each is a divergence: the chain runs to completion with info 0."""
    rng = np.random.default_rng(21)
    N, d = 24, 2
    half = rng.uniform(-3.0, 3.0, (N // 2, d))
    Xdup = np.concatenate([half, half])
    X = np.stack([Xdup, rng.uniform(-3.0, 3.0, (N, d))])
    Y = np.stack([1e-13 * np.sin(Xdup.sum(1)), np.sin(X[1].sum(1)) + 0.2 * rng.standard_normal(N)])
    Xd, Yd = dev(X, engine), dev(Y, engine)
    start = np.array([[0.0, 0.0, -30.0, -40.0], [0.5, 0.6, 0.1, -0.3]])
    # the factorisation holds at the start and fails ten units of log sig_n below it, or with sig_f back at 1
    probe = np.array([start[0], [0.0, 0.0, -30.0, -50.0], [0.0, 0.0, 0.0, -40.0]])
    lp, _ = logp_batch(engine, Xd, Yd, probe, [0, 0, 0], [0, 0, 0])
    assert np.isfinite(lp[0]) and lp[1] == -np.inf and lp[2] == -np.inf, lp
    r = engine.exact_nuts_batch(Xd, Yd, start, [31, 32], 5, 20, ix=[0, 1], iy=[0, 1], max_treedepth=6)
    div = r["stats"][:, :, 4].numpy()
    print("diverging draws: %s of 20; evaluations %s; last position %s" % (div.sum(1).tolist(), r["evaluations"].tolist(),
                                                                         r["samples"][0, -1].tolist()))
    assert r["info"].tolist() == [0, 0] and r["draws"].tolist() == [25, 25]
    assert div[0].sum() >= 1 and np.isfinite(r["samples"].numpy()).all() and np.isfinite(r["stats"][:, :, 6].numpy()).all()
    assert r["samples"][0, -1, 3] < -41.0   # the chain has moved towards the edge: these are not trajectories thrown out of range
    alone = engine.exact_nuts_batch(Xd[1].contiguous(), Yd[1].contiguous(), start[1:], [32], 5, 20, max_treedepth=6)
    assert np.array_equal(bits(alone), bits(r, slice(1, 2)))


def test_quadrature_posterior_pin_on_the_device(engine):
    """tests/test_exact_nuts.py's pin with the real engine: same chains, same check_moments, same 4 MCSE."""
    from test_gpr_hmc import pin_data, quadrature_posterior
    from test_posterior_pin import check_moments
    th, diverging = pin_run(engine)
    assert diverging <= 0.01
    check_moments(th, quadrature_posterior(*pin_data()), "sample_exact_nuts_batch / device")


def test_occupancy_and_refusals(engine):
    lib = engine.exact_nuts_lib
    for k in range(3):  # chains per CU
        assert [lib.sgp_exact_nuts_batch_occupancy(N, k) for N in (1, 32, 33, 64, 65, 128)] == [2, 2, 2, 2, 1, 1], k
    assert lib.sgp_exact_nuts_batch_occupancy(129, 0) == -2 and lib.sgp_exact_nuts_batch_occupancy(10, 3) == -1
    ok = dict(X=torch.zeros(1, 10, 2), Y=torch.zeros(1, 10), q0=np.zeros((1, 4)), kernel="rbf", max_treedepth=10)
    for bad, status in [(dict(X=torch.zeros(1, 129, 2), Y=torch.zeros(1, 129)), -2), (dict(X=torch.zeros(1, 10, 9), q0=np.zeros((1, 11))), -2),
                        (dict(kernel="composite"), -1), (dict(max_treedepth=12), -1)]:
        a = dict(ok, **bad)
        with pytest.raises(ggp_amd.SgpStatusError) as e:
            engine.exact_nuts_batch(dev(a["X"], engine), dev(a["Y"], engine), a["q0"], [1], 2, 2, kernel=a["kernel"],
                                    max_treedepth=a["max_treedepth"])
        assert e.value.status == status, bad


def test_gpr_hmc_device_sampler_end_to_end(engine, capsys):
    rng = np.random.default_rng(100)
    X = rng.standard_normal((120, 2))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(120)
    Xtr, ytr, Xte = X[:100], y[:100], X[100:]
    m = ggp_amd.GPR_HMC(dev(Xtr, engine), dev(ytr, engine), ggp_amd.GaussianLikelihood(), engine=engine, seed=3, device_sampler=True)
    trace, step, perf = m.train_model()
    assert len(trace) == 10 and trace.device_resident and step[0] > 0 and perf[0] > 0
    preds = ggp_amd.full_mixture_posterior_predictive(m, dev(Xte, engine), trace)
    assert len(preds) == 10, capsys.readouterr().out
    dbl = ExactDouble()
    for i, p in enumerate(preds):
        th = trace[i]
        ls, sf2, s2 = list(np.asarray(th["ls"]).reshape(-1)), float(th["sig_f"]) ** 2, float(th["sig_n"]) ** 2
        rr = dbl.exact_eval(T(Xtr), T(ytr), ls, sf2, s2, want_grad=False, want_factors=True)
        mr, _, cr = dbl.exact_predict(T(Xte), T(Xtr), ls, sf2, s2, rr["factors"], full_cov=True)
        assert float((p.loc.cpu() - mr).abs().max()) <= 1e-9 * max(1.0, float(mr.abs().max())), i
        assert float((p.covariance_matrix.cpu() - cr).abs().max()) <= 1e-9 * max(1.0, float(cr.abs().max())), i
