"""GPU: the batched device-resident NUTS over the collapsed sparse-GP bound (csrc/sgp_vfe_nuts.hip) -- the device chain against the
host-driven one in every size class (more than one row tile per class, M > N), its logp column against the batched evaluation, and that
nothing but the per-draw seconds depends on how the run is cut into launches, on what else shares the batch, on the call, the stream or
the context; bad starts, divergences, the posterior pin, occupancy and refusals, and fit_sgpr_batch(...).sample_nuts(...) end to end."""
import numpy as np
import pytest
import torch

from conftest import dev, load_golden
from test_vfe_nuts import pin_run
from vfe_nuts_double import VfeNutsDouble

import ggp_amd
import ggp_amd._lib as L
from ggp_amd.sgpr_nuts import vfe_logp_batch

pytestmark = pytest.mark.gpu

# (N, M, d, kernel): N = 1; M > N; class 16 over two tiles of 128 rows; class 32 over two tiles of 64; class 32 at its upper edge; class 64
# over two tiles of 32; class 64 at its upper edge over four tiles
CELLS = [(1, 1, 1, "rbf"), (5, 9, 1, "rbf"), (129, 16, 1, "rbf"), (65, 17, 2, "matern32"), (70, 32, 3, "matern52"), (33, 33, 8, "rbf"),
         (97, 64, 2, "matern32")]
TUNE, DRAWS, DEPTH = 20, 15, 6
KEYS = ("samples", "stats", "evaluations", "draws", "info")
CELL_ID = lambda c: "N%d-M%d-d%d-%s" % c  # noqa: E731


def bits(r, rows=slice(None)):
    """Everything a run returns but the per-draw seconds, as integers."""
    return np.concatenate([np.ascontiguousarray(np.asarray(r[k])[rows]).reshape(-1).view(
        {8: np.uint64, 4: np.uint32}[np.asarray(r[k]).dtype.itemsize]).astype(np.uint64) for k in KEYS])


def problem(N, M, d, seed):
    """A data set whose chain two samplers can be compared on.  Device and host differ by an ulp in exp / log and by the device's fused
    multiply-adds at every leapfrog, and a NUTS chain amplifies such differences from draw to draw; the comparison below means
    something only while they stay under its tolerance.  The target therefore depends on the first input alone (one lengthscale the
    data identify, the others left to the prior).  Measured on the CPU double, with the theta row of every evaluation of ONE of two
    host-driven chains moved by an ulp at random: on this rule the two chains of every cell keep identical trees and end within 1.4e-9
    relative, a factor 70 inside the tolerance -- whereas with a target sin(sum of all inputs) the two HOST chains of the d = 8 cell
    part (884 against 876 evaluations), which says nothing about the device."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3.0, 3.0, (N, d))
    y = np.sin(X[:, 0]) + 0.2 * rng.standard_normal(N)
    Z = X[rng.permutation(N)[:M]].copy() if M <= N else rng.uniform(-3.0, 3.0, (M, d))
    q0 = np.array([np.log(2.0)] * d + [0.0, 0.0]) + rng.uniform(-0.3, 0.3, d + 2)
    return X, y, Z, q0


_RUNS = {}


def cell_run(engine, cell):
    """The device chain of a cell (computed once, shared by the tests below, never modified)."""
    if cell not in _RUNS:
        N, M, d, kernel = cell
        X, y, Z, q0 = problem(N, M, d, 1000 * N + 10 * M + d)
        seed = 7000 + 100 * M + N
        Xd, yd, Zd = dev(X, engine), dev(y, engine), dev(Z, engine)
        r = engine.vfe_nuts_batch(Xd, yd, Zd, q0[None], [seed], TUNE, DRAWS, kernel=kernel, max_treedepth=DEPTH)
        _RUNS[cell] = (Xd, yd, Zd, q0, seed, r)
    return _RUNS[cell]


@pytest.mark.parametrize("cell", CELLS, ids=CELL_ID)
def test_device_chain_is_the_host_driven_chain(engine, cell):
    """hmc.NUTS(rng=SplitMix(seed)) over engine.vfe_eval_batch (P = 1) + theta_logp_and_grad from the same q0: identical trees, draws
    equal to rounding (the tolerances tests/test_exact_nuts_gpu.py holds the exact sampler to: the device's exp is within an ulp of
    libm's)."""
    N, M, d, kernel = cell
    Xd, yd, Zd, q0, seed, r = cell_run(engine, cell)
    assert int(r["info"][0]) == 0 and int(r["draws"][0]) == TUNE + DRAWS
    h = VfeNutsDouble(evaluator=engine).vfe_nuts_batch(Xd, yd, Zd, q0[None], [seed], TUNE, DRAWS, kernel=kernel, max_treedepth=DEPTH)
    assert int(h["info"][0]) == 0
    print("N=%d M=%d d=%d %s: %d evaluations in %d launches, tree sizes %s" % (N, M, d, kernel, int(r["evaluations"][0]), r["launches"],
                                                                             r["stats"][0, :, 1].tolist()))
    assert int(r["evaluations"][0]) == int(h["evaluations"][0])
    assert np.array_equal(r["stats"][0, :, 1].numpy(), h["stats"][0, :, 1].numpy())
    assert np.array_equal(r["stats"][0, :, 7].numpy(), h["stats"][0, :, 7].numpy())
    assert np.allclose(r["stats"][0, :, 0].numpy(), h["stats"][0, :, 0].numpy(), rtol=1e-9, atol=0.0)
    assert np.allclose(r["samples"][0].numpy(), h["samples"][0].numpy(), rtol=1e-7, atol=1e-9)
    assert np.all(r["seconds"].numpy() > 0.0)


@pytest.mark.parametrize("cell", CELLS, ids=CELL_ID)
def test_logp_column_is_the_batched_evaluation_at_the_draw(engine, cell):
    """vfe_eval_batch at exp(sample) + prior + Jacobian, within 1e-10 (|logp| + N): the project's bound for this statement."""
    N, M, d, kernel = cell
    Xd, yd, Zd, _, _, r = cell_run(engine, cell)
    lp = r["stats"][0, :, 6].numpy()
    ref = vfe_logp_batch(engine, Xd, yd, Zd, r["samples"][0].numpy(), None, None, None, kernel, 1e-6)
    print("N=%d M=%d d=%d %s: max |logp - ref| / (|ref| + N) = %.3g" % (N, M, d, kernel, np.max(np.abs(lp - ref) / (np.abs(ref) + N))))
    assert np.isfinite(ref).all() and np.all(np.abs(lp - ref) <= 1e-10 * (np.abs(ref) + N))


@pytest.mark.parametrize("cell", [(33, 33, 8, "rbf"), (97, 64, 2, "matern32")], ids=CELL_ID)
def test_the_result_does_not_depend_on_evals_per_launch(engine, cell):
    N, M, d, kernel = cell
    Xd, yd, Zd, q0, seed, r = cell_run(engine, cell)   # the default
    launches = [r["launches"]]
    for epl in (1, 5):
        c = engine.vfe_nuts_batch(Xd, yd, Zd, q0[None], [seed], TUNE, DRAWS, kernel=kernel, max_treedepth=DEPTH, evals_per_launch=epl)
        assert np.array_equal(bits(c), bits(r)), epl
        launches.append(c["launches"])
    evals = int(r["evaluations"][0])
    print("N=%d M=%d: %d evaluations in %s launches (default, 1, 5 per launch)" % (N, M, evals, launches))
    assert launches[1] >= evals and evals / 5 <= launches[2] < launches[1]


def batch_problem():
    rng = np.random.default_rng(77)
    N, M, d, nX, nY, nZ, C = 30, 6, 2, 7, 5, 3, 600
    X = rng.uniform(-3.0, 3.0, (nX, N, d))
    Y = np.sin(X.sum(2))[rng.integers(0, nX, nY)] + 0.3 * rng.standard_normal((nY, N))
    Z = rng.uniform(-3.0, 3.0, (nZ, M, d))
    ix, iy, iz = (rng.integers(0, n, C).astype(np.int32) for n in (nX, nY, nZ))
    q0 = np.array([np.log(2.0)] * d + [0.0, 0.0]) + rng.uniform(-0.5, 0.5, (C, d + 2))
    seeds = [int(s) for s in rng.integers(1, 2 ** 62, C)]
    return X, Y, Z, ix, iy, iz, q0, seeds


def test_a_chain_of_a_batch_is_the_chain_alone_on_every_call_stream_and_context(engine):
    """600 chains -- more than the chip holds at once -- over 7 data sets x 5 targets x 3 inducing sets with scrambled ix / iy / iz."""
    X, Y, Z, ix, iy, iz, q0, seeds = batch_problem()
    Xd, Yd, Zd = dev(X, engine), dev(Y, engine), dev(Z, engine)
    kw = dict(kernel="matern32", max_treedepth=6)
    r = engine.vfe_nuts_batch(Xd, Yd, Zd, q0, seeds, 10, 8, ix=ix, iy=iy, iz=iz, **kw)
    assert (r["info"] == 0).all() and (r["draws"] == 18).all() and np.isfinite(r["samples"].numpy()).all()
    for c in (0, 299, 599):
        one = engine.vfe_nuts_batch(Xd[ix[c]].contiguous(), Yd[iy[c]].contiguous(), Zd[iz[c]].contiguous(), q0[c:c + 1], seeds[c:c + 1], 10, 8,
                                    **kw)
        assert np.array_equal(bits(one), bits(r, slice(c, c + 1))), c
    whole = bits(r)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        again = engine.vfe_nuts_batch(Xd, Yd, Zd, q0, seeds, 10, 8, ix=ix, iy=iy, iz=iz, **kw)
    stream.synchronize()
    assert np.array_equal(bits(again), whole)
    other = ggp_amd.HipEngine(own_context=True)
    assert np.array_equal(bits(other.vfe_nuts_batch(Xd, Yd, Zd, q0, seeds, 10, 8, ix=ix, iy=iy, iz=iz, evals_per_launch=7, **kw)), whole)


def test_bad_starts_are_reported_and_touch_nothing_else(engine):
    X, y, Z, q = problem(20, 5, 2, 5)
    Xd, yd, Zd = dev(X, engine), dev(y, engine), dev(Z, engine)
    rng = np.random.default_rng(8)
    q0 = q + rng.uniform(-0.2, 0.2, (8, 4))
    q0[2, 1] = float("nan")
    q0[5, 3] = -301.0
    seeds = list(range(50, 58))
    r = engine.vfe_nuts_batch(Xd, yd, Zd, q0, seeds, 10, 6, max_treedepth=6)
    bad = np.zeros(8, dtype=bool)
    bad[[2, 5]] = True
    assert np.array_equal(r["info"].numpy(), np.where(bad, L.VFE_NUTS_BAD_START, 0))
    for k in ("samples", "stats", "seconds"):
        assert np.isnan(r[k].numpy()[bad]).all() and np.isfinite(r[k].numpy()[~bad]).all(), k
    assert (r["draws"].numpy()[bad] == 0).all() and (r["evaluations"].numpy()[bad] == 1).all() and (r["draws"].numpy()[~bad] == 16).all()
    six = engine.vfe_nuts_batch(Xd, yd, Zd, q0[~bad], [s for s, b in zip(seeds, bad) if not b], 10, 6, max_treedepth=6)
    assert np.array_equal(bits(six), bits(r, ~bad))


def test_failed_factorisations_are_divergences_not_errors(engine):
    """Two identical rows of Z with a jitter of 1e-14: the duplicate's pivot of chol(K_uu) is about 2 jitter, against the gate
    8 M 2^-53 (sig_f^2 + jitter).  The density is finite at log sig_f = 0 and has no finite value above sig_f ~ 2.4 -- which is where
    targets of amplitude 10 pull the chain.  Each evaluation beyond that wall reports the kernel's info code and is a divergence for the
    sampler: the chain runs to completion with info 0."""
    rng = np.random.default_rng(21)
    N, jitter = 20, 1e-14
    X = np.sort(rng.uniform(-3.0, 3.0, (N, 1)), 0)
    Y = np.stack([10.0 * np.sin(X[:, 0]) + 0.3 * rng.standard_normal(N), np.sin(X[:, 0]) + 0.2 * rng.standard_normal(N)])
    Z = np.array([[[-2.0], [0.5], [0.5], [2.0]], [[-2.0], [-0.7], [0.7], [2.0]]])
    Xd, Yd, Zd = dev(X, engine), dev(Y, engine), dev(Z, engine)
    start = np.array([[0.0, 0.0, 0.0], [0.3, 0.1, -0.5]])
    # the premise: finite at the start, no finite density beyond the wall (log sig_f = 1.5 and 2.5: sig_f = 4.5 and 12)
    probe = np.array([start[0], [0.0, 1.5, 0.0], [0.0, 2.5, 0.0]])
    lp = vfe_logp_batch(engine, Xd, Yd, Zd, probe, None, [0, 0, 0], [0, 0, 0], "rbf", jitter)
    assert np.isfinite(lp[0]) and lp[1] == -np.inf and lp[2] == -np.inf, lp
    r = engine.vfe_nuts_batch(Xd, Yd, Zd, start, [31, 32], 5, 20, iy=[0, 1], iz=[0, 1], jitter=jitter, max_treedepth=6)
    div = r["stats"][:, :, 4].numpy()
    print("diverging draws: %s of 20; evaluations %s; last position %s" % (div.sum(1).tolist(), r["evaluations"].tolist(),
                                                                         r["samples"][0, -1].tolist()))
    assert r["info"].tolist() == [0, 0] and r["draws"].tolist() == [25, 25]
    assert np.isfinite(r["samples"].numpy()).all() and np.isfinite(r["stats"][:, :, 6].numpy()).all()
    assert div[0].sum() >= 1
    alone = engine.vfe_nuts_batch(Xd, Yd[1].contiguous(), Zd[1].contiguous(), start[1:], [32], 5, 20, jitter=jitter, max_treedepth=6)
    assert np.array_equal(bits(alone), bits(r, slice(1, 2)))


def test_quadrature_posterior_pin_on_the_device(engine):
    """tests/test_vfe_nuts.py's pin with the real engine: same chains, same check_moments, same 4 MCSE."""
    from test_posterior_pin import check_moments
    th, diverging = pin_run(engine)
    assert diverging <= 0.01
    check_moments(th, load_golden("posterior_rbf_d1_tiny"), "sample_sgpr_nuts_batch / device")


def test_occupancy_and_refusals(engine):
    lib = engine.vfe_nuts_lib
    for k in range(3):
        occ = [lib.sgp_vfe_nuts_batch_occupancy(M, k) for M in (1, 16, 17, 32, 33, 64)]
        print("kernel %d: chains per CU by M = 1, 16, 17, 32, 33, 64: %s" % (k, occ))
        assert min(occ) >= 1, (k, occ)
        assert engine.vfe_nuts_evals_per_launch(1, 65536, 64, ("rbf", "matern32", "matern52")[k]) >= 1
    assert lib.sgp_vfe_nuts_batch_occupancy(65, 0) == -2 and lib.sgp_vfe_nuts_batch_occupancy(10, 3) == -1
    # the default shrinks with N and with the number of waves of workgroups
    e = engine.vfe_nuts_evals_per_launch
    assert e(1, 200, 25) > e(1, 20000, 25) > e(1, 65536, 25) >= 1 and e(1, 200, 25) > e(100000, 200, 25) >= 1
    z = lambda *s: dev(np.zeros(s), engine)  # noqa: E731
    with pytest.raises(ValueError, match="M <= 64"):
        engine.vfe_nuts_batch(z(10, 2), z(10), z(65, 2), np.zeros((1, 4)), [1], 2, 2)
    for bad, status in [(dict(kernel="composite"), -1), (dict(max_treedepth=12), -1), (dict(jitter=-1.0), -1), (dict(evals_per_launch=0), -1)]:
        with pytest.raises(ggp_amd.SgpStatusError) as err:
            engine.vfe_nuts_batch(z(10, 2), z(10), z(5, 2), np.zeros((1, 4)), [1], 2, 2, **bad)
        assert err.value.status == status, bad


def test_fit_then_sample_end_to_end(engine, capsys):
    rng = np.random.default_rng(100)
    B, N, M = 3, 40, 6
    X = rng.uniform(-2.0, 2.0, (B, N + 8, 2))
    Y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, N + 8))
    fit = ggp_amd.fit_sgpr_batch(X[:, :N], Y[:, :N], X[:, :M].copy(), max_steps=30, lr=0.05, seed=0, engine=engine)
    post = fit.sample_nuts(8, 12, chains=2, seed=3, max_treedepth=6)
    assert (post.info == 0).all() and (post.draws == 20).all() and post.samples.shape == (B, 2, 8, 4) and np.isfinite(post.samples).all()
    assert post.launches >= 1 and post.seconds.shape == (B, 2, 8) and (post.seconds > 0).all()
    for b in range(B):
        for c in range(2):
            tr = post.traces[b][c]
            assert len(tr) == 8 and np.asarray(tr["ls"]).shape == (8, 2) and np.asarray(tr["sig_f"]).shape == (8,) and tr.device_resident
        m = post.model(b)
        assert isinstance(m, ggp_amd.BayesianSparseGPR_HMC)
        preds = ggp_amd.mixture_posterior_predictive(m, dev(X[b, N:], engine), post.traces[b][1])
        assert 1 <= len(preds) <= 8, capsys.readouterr().out
        for p in preds:
            assert p.mean.shape == (8,) and bool(torch.isfinite(p.mean).all()) and bool(torch.isfinite(p.variance).all())
            assert bool((p.variance > 0).all())
