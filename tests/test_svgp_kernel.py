"""The SVGP kernels (csrc/sgp_svgp.hip) against the long-double reference tests/svgp_reference.py at edge shapes.

Every (B, M, d) cell is the smallest shape that reaches its branch:

    (1, 1, 1)        the smallest shape                          (257, 128, 8)   the 256-lane stride of svgp_kub_bwd_kernel; M = Mp
    (63, 5, 1)       B < 64 (and the ill-conditioned cell)       (300, 129, 9)   Mp = 256 with 127 padded rows; d > 8
    (64, 64, 2)      the 64 boundaries                           (200, 130, 32)  SGP_MAX_DIM
    (65, 65, 3)      one past them                               (1400, 300, 2)  Mp = 384 (an odd number of 128-blocks); Mp Bp > 524 288
    (16385, 5, 1)    second stride of the ELL kernel             (64, 5, 1)      the Bernoulli tail: z < -39.1, past erfc's underflow

Every cell keeps rows of Z equal to rows of X (r = 0).  The comparison is component-wise |got - ref| <= tolerance(cell) * A with A the
reference's condition scale and

    tolerance = MARGIN * max(e64, FLOOR),   MARGIN = 10, FLOOR = 1e-13,

e64 the cell's float64 level: the worst |fp64 - ref| / A of the fp64 oracle and of a float64 run of the closed form, measured on the
CPU (tests/test_svgp_reference.py recomputes the table below and shows that five deliberate defects stand 100x above the tolerance).
10: the device multiplies by an explicit L^-1 where the oracle substitutes, DESIGN section 4a item 1 finds the two within an order of
magnitude of each other.

Not covered here: the 256-block cap of svgp_kub_bwd_reduce_kernel (needs M d > 65 536); the mixture-predictive kernels mix_* have
edge-shape tests of their own (tests/test_gpu_parity.py).

The (1400, 300, 2) cases take ~10 s each: 9 of them are the long-double reference (numpy has no BLAS for that type).
"""
import numpy as np
import pytest
import torch

import svgp_reference as R

MARGIN = 10
FLOOR = 1e-13
# e64 per (B, M, d, kernel, likelihood): measured by tests/test_svgp_reference.py::measure_e64, one significant digit
E64 = {
    (1, 1, 1, 'rbf', 'gaussian'): 2e-16,
    (1, 1, 1, 'rbf', 'bernoulli'): 2e-16,
    (1, 1, 1, 'matern32', 'gaussian'): 9e-17,
    (1, 1, 1, 'matern32', 'bernoulli'): 2e-16,
    (1, 1, 1, 'matern52', 'gaussian'): 9e-17,
    (1, 1, 1, 'matern52', 'bernoulli'): 2e-16,
    (63, 5, 1, 'rbf', 'gaussian'): 3e-17,
    (63, 5, 1, 'rbf', 'bernoulli'): 5e-18,
    (63, 5, 1, 'matern32', 'gaussian'): 7e-17,
    (63, 5, 1, 'matern32', 'bernoulli'): 5e-18,
    (63, 5, 1, 'matern52', 'gaussian'): 2e-17,
    (63, 5, 1, 'matern52', 'bernoulli'): 5e-18,
    (64, 64, 2, 'rbf', 'gaussian'): 1e-15,
    (64, 64, 2, 'rbf', 'bernoulli'): 3e-16,
    (64, 64, 2, 'matern32', 'gaussian'): 8e-16,
    (64, 64, 2, 'matern32', 'bernoulli'): 2e-16,
    (64, 64, 2, 'matern52', 'gaussian'): 1e-15,
    (64, 64, 2, 'matern52', 'bernoulli'): 2e-16,
    (65, 65, 3, 'rbf', 'gaussian'): 1e-16,
    (65, 65, 3, 'rbf', 'bernoulli'): 7e-17,
    (65, 65, 3, 'matern32', 'gaussian'): 3e-16,
    (65, 65, 3, 'matern32', 'bernoulli'): 7e-17,
    (65, 65, 3, 'matern52', 'gaussian'): 4e-16,
    (65, 65, 3, 'matern52', 'bernoulli'): 7e-17,
    (257, 128, 8, 'rbf', 'bernoulli'): 1e-16,
    (257, 128, 8, 'matern52', 'gaussian'): 1e-16,
    (300, 129, 9, 'rbf', 'bernoulli'): 3e-17,
    (300, 129, 9, 'matern52', 'gaussian'): 3e-16,
    (200, 130, 32, 'rbf', 'bernoulli'): 1e-16,
    (200, 130, 32, 'matern52', 'gaussian'): 4e-16,
    (1400, 300, 2, 'rbf', 'bernoulli'): 2e-16,
    (1400, 300, 2, 'matern52', 'gaussian'): 7e-16,
    (16385, 5, 1, 'rbf', 'gaussian'): 3e-16,
    (16385, 5, 1, 'rbf', 'bernoulli'): 1e-16,
    (16385, 5, 1, 'matern32', 'gaussian'): 5e-16,
    (16385, 5, 1, 'matern32', 'bernoulli'): 2e-16,
    (16385, 5, 1, 'matern52', 'gaussian'): 5e-16,
    (16385, 5, 1, 'matern52', 'bernoulli'): 2e-16,
    (64, 5, 1, 'rbf', 'bernoulli', 'tail'): 5e-15,
}
BATCH_COMBOS = {(65, 65, 3): [("rbf", "gaussian"), ("matern52", "bernoulli")], (300, 129, 9): [("rbf", "bernoulli"), ("matern52", "gaussian")]}
PREDICT_CELL = (300, 129, 9)
TAIL_KEY = (*R.TAIL_CELL, "rbf", "bernoulli", "tail")


def all_cells():
    return [(*cell, kernel, lik) for cell in R.CELLS for kernel, lik in R.combos(cell)] + [TAIL_KEY]


def tolerance(key):
    return MARGIN * max(E64[key], FLOOR)


def dev(a, engine):
    return torch.as_tensor(np.array(a, dtype=np.float64)).to(engine.device).contiguous()


def unpack(res, k=None):
    """The device result as the reference's keys (sample k of a batch result)."""
    pick = (lambda t: t.cpu()) if k is None else (lambda t: t[k].cpu())
    out = pick(res["out"])
    got = {"elbo": out[0], "ell_sum": out[1], "kl": out[2]}
    got.update({key: pick(res[key]) for key in ("g_m", "g_LS", "g_Z", "g_ls", "g_sf2", "g_s2") if key in res})
    return got


def check(what, got, ref, A, tol):
    """Prints every figure as a multiple of the tolerance, then asserts."""
    w = {k: v / tol for k, v in R.worst(got, ref, A, keys=[k for k in R.KEYS + ("mu", "v") if k in got]).items()}
    print("SVGP_KERNEL %s worst |got - ref| / (tol A) = %.3g  %s" % (what, max(w.values()), {k: "%.2g" % v for k, v in w.items()}))
    assert max(w.values()) <= 1.0, (what, w)
    return max(w.values())


def single(engine, inp, kernel, lik, with_grads, ls=None, sf2=None, s2=None):
    return engine.svgp_elbo(dev(inp["X"], engine), dev(inp["y"], engine), dev(inp["Z"], engine), list(inp["ls"] if ls is None else ls),
                            inp["sf2"] if sf2 is None else sf2, inp["s2"] if s2 is None else s2, dev(inp["m"], engine), dev(inp["LS"], engine),
                            inp["N_total"], jitter=inp["jitter"], kernel=kernel, likelihood=lik, with_grads=with_grads)


def batch(engine, inp, kernel, lik, with_grads, ls, sf2, s2):
    return engine.svgp_elbo_batch(dev(inp["X"], engine), dev(inp["y"], engine), dev(inp["Z"], engine), ls.tolist(), sf2.tolist(), s2.tolist(),
                                  dev(inp["m"], engine), dev(inp["LS"], engine), inp["N_total"], jitter=inp["jitter"], kernel=kernel,
                                  likelihood=lik, with_grads=with_grads)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [k for k in all_cells() if k != TAIL_KEY], ids=lambda k: "-".join(str(v) for v in k))
def test_svgp_elbo_vs_long_double(engine, key):
    """sgp_svgp_elbo: the bound, sum E log p, KL and all six gradients; the value-only call returns the same bits."""
    B, M, d, kernel, lik = key
    inp = R.cell_inputs(B, M, d, lik)
    ref, A = R.cell_reference(B, M, d, kernel, lik)
    res = single(engine, inp, kernel, lik, True)
    assert int(res["info"].item()) == 0
    check("elbo %s" % (key,), unpack(res), ref, A, tolerance(key))
    val = single(engine, inp, kernel, lik, False)
    assert torch.equal(val["out"], res["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("cell,kernel,lik", [(c, k, l) for c, kl in BATCH_COMBOS.items() for k, l in kl])
def test_svgp_elbo_batch_vs_long_double(engine, cell, kernel, lik, S):
    """sgp_svgp_elbo_batch: every hyper-parameter sample against the reference at that sample."""
    inp = R.cell_inputs(*cell, lik)
    ls, sf2, s2 = R.theta_samples(inp, S)
    res = batch(engine, inp, kernel, lik, True, ls, sf2, s2)
    assert res["info"].cpu().tolist() == [0] * S
    for k in range(S):
        ref, A = R.cell_reference(*cell, kernel, lik, S=S, k=k)
        check("batch %s S=%d k=%d" % ((*cell, kernel, lik), S, k), unpack(res, k), ref, A, tolerance((*cell, kernel, lik)))
    val = batch(engine, inp, kernel, lik, False, ls, sf2, s2)
    assert torch.equal(val["out"], res["out"])


def predict_tolerance(kernel):
    return tolerance((*PREDICT_CELL, kernel, "bernoulli" if kernel == "rbf" else "gaussian"))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 64, 65])
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_svgp_predict_vs_long_double(engine, kernel, T):
    """sgp_svgp_predict at the cell (., 129, 9): latent mean and variance at T test rows (the first three are rows of Z)."""
    inp = R.cell_inputs(*PREDICT_CELL, "gaussian")
    Xs = inp["X"][:T]
    (mu_r, v_r), (a_mu, a_v) = R.predict_reference(Xs, inp["Z"], inp["ls"], inp["sf2"], inp["m"], inp["LS"], inp["jitter"], kernel)
    mu, v, info = engine.svgp_predict(dev(Xs, engine), dev(inp["Z"], engine), list(inp["ls"]), inp["sf2"], dev(inp["m"], engine),
                                      dev(inp["LS"], engine), jitter=inp["jitter"], kernel=kernel)
    assert int(info.item()) == 0 and mu.shape == (T,) and v.shape == (T,)
    check("predict %s T=%d" % (kernel, T), {"mu": mu, "v": v}, {"mu": mu_r, "v": v_r}, {"mu": a_mu, "v": a_v}, predict_tolerance(kernel))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["rbf", "matern52"])
def test_svgp_predict_batch_vs_long_double(engine, kernel):
    """svgp_predict_batch at the same cell: T = 70 rows in chunks of 32 (two full, one of 6), three hyper-parameter samples."""
    inp = R.cell_inputs(*PREDICT_CELL, "gaussian")
    Xs = inp["X"][:70]
    ls, sf2, _ = R.theta_samples(inp, 3)
    try:
        engine.SVGP_PREDICT_CHUNK = 32
        mu, v, info = engine.svgp_predict_batch(dev(Xs, engine), dev(inp["Z"], engine), ls.tolist(), sf2.tolist(), dev(inp["m"], engine),
                                                dev(inp["LS"], engine), jitter=inp["jitter"], kernel=kernel)
    finally:
        del engine.SVGP_PREDICT_CHUNK
    assert info.cpu().tolist() == [0, 0, 0] and mu.shape == (3, 70)
    for k in range(3):
        (mu_r, v_r), (a_mu, a_v) = R.predict_reference(Xs, inp["Z"], ls[k], sf2[k], inp["m"], inp["LS"], inp["jitter"], kernel)
        check("predict_batch %s k=%d" % (kernel, k), {"mu": mu[k], "v": v[k]}, {"mu": mu_r, "v": v_r}, {"mu": a_mu, "v": a_v},
              predict_tolerance(kernel))


@pytest.mark.gpu
def test_svgp_bernoulli_tail_is_finite(engine):
    """Cell (64, 5, 1), Bernoulli: three labels flipped against a mean of ~ +30, sqrt(v) ~ 1.3, so the outer Gauss-Hermite node has
    z <= -39.1, where 0.5 erfc(-z / sqrt 2) is 0 in binary64 and log of it -inf.  log Phi(-39.1) ~ -769 is finite: the single and the
    batch entry must return the bound and the gradients within the cell's tolerance.
    With log(0.5 erfc(.)) in log_ndtr_dev (before the erfcx form) both entries returned -inf here."""
    B, M, d, kernel, lik, _ = TAIL_KEY
    inp = R.tail_inputs()
    ref, A = R.cell_reference(B, M, d, kernel, lik, tail=True)
    assert ref["zmin"] <= -39.1, ref["zmin"]            # on the reference, not on the device
    assert np.isfinite(float(ref["elbo"]))
    tol = tolerance(TAIL_KEY)
    res = single(engine, inp, kernel, lik, True)
    print("SVGP_KERNEL tail single bound = %r (reference %.17g, zmin %.3f)" % (float(res["out"][0]), float(ref["elbo"]), ref["zmin"]))
    assert int(res["info"].item()) == 0 and bool(torch.isfinite(res["out"]).all())
    check("tail single", unpack(res), ref, A, tol)
    one = np.array([inp["sf2"]]), np.array([inp["s2"]])
    resb = batch(engine, inp, kernel, lik, True, inp["ls"][None, :], *one)
    print("SVGP_KERNEL tail batch bound = %r" % float(resb["out"][0, 0]))
    assert resb["info"].cpu().tolist() == [0] and bool(torch.isfinite(resb["out"]).all())
    check("tail batch", unpack(resb, 0), ref, A, tol)
