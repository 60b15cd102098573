"""GPU: the streaming posterior predictive against the long-double reference tests/vfe_predict_reference.py (STREAM_CELLS) --

    sgp_predict              csrc/sgp_tail.hip (kus_kernel / comp_kmatrix, the two masked gemms, pred_cols_kernel, pred_cov_kernel,
                             pred_cov_add_kernel) from the ``factors`` of CollapsedBound(form="whitened") and form="streaming": mean, var and
                             the full covariance at every cell its form is run at, with and without the noise; past its test-row chunk
                             (T = 16385, and the mixture route's 8193) mean and var, the leading rows bit for bit those of a short call
    sgp_mixture_predict      csrc/sgp_svgp.hip (mixture_predict_impl and the mix_* kernels) at nine draws theta_k = theta (1 + 0.05 k) --
                             two batches --, with the covariance and the PSD gate and without, each draw against the reference at its own
                             theta_k; the ``ill`` cells; T = 8193 without a covariance
    sgp_mixture_predict_zs   the same with inducing inputs Z_k = Z + 0.01 k noise_k of their own per draw
    leading dimensions       ldx = d + 2, ldxs = d + 3, ldz = d + 1 through the C ABI, NaN in the padding: the bits of the contiguous call

component-wise |got - ref| <= 10 max(e64, 1e-13) S (see tests/test_stream_predict.py, whose ``check_*`` functions run here on the
device; e64 comes from float64 runs of the reference on the host, never from the device).  Every test prints STREAM_PREDICT lines: per
cell and route the worst |got - ref| / S of each output beside its tolerance.

Measured on an MI355X (profiles/stream_predict_anchor.json, written by tools/stream_predict_ratios.py from these same checks).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import vfe_predict_reference as R
from conftest import dev
from test_stream_predict import GATE_JITTER, ZS_CELL, check_mixture_cell, check_predict_big_t, check_predict_cell, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,form", [(n, f) for f in R.ROUTES for n in R.stream_cells(f)])
def test_predict_from_factors_matches_the_long_double_reference(engine, name, form):
    out = check_predict_cell(engine, lambda a: dev(a, engine), name, form)
    assert ("predict_%s_noise_free" % form in out) == (name in ("300-65-2-rbf", "200-64-2-matern52"))


@pytest.mark.parametrize("form", R.ROUTES)
def test_predict_past_the_test_row_chunks(engine, form):
    """T = 8193 and T = 16385 without a covariance: sgp_predict's row loop takes a second pass at the latter, of one row."""
    check_predict_big_t(engine, lambda a: dev(a, engine), form, bits=True)


@pytest.mark.parametrize("name", R.STREAM_STATIONARY)
def test_mixture_predict_matches_the_long_double_reference_draw_by_draw(engine, name):
    assert R.DRAWS == 9 > engine.MIXTURE_BATCH == 8
    assert sorted(check_mixture_cell(engine, lambda a: dev(a, engine), name)) == ["mixture", "mixture_cov"]


def test_mixture_predict_past_the_test_row_chunk(engine):
    """T = 8193 without a covariance: mixture_predict_impl's test-side loop takes a second pass, of one row (the far point)."""
    assert sorted(check_mixture_cell(engine, lambda a: dev(a, engine), R.BIG_T_CELL, T=R.BIG_T[0])) == ["mixture"]


def test_mixture_predict_with_inducing_inputs_per_draw(engine):
    assert sorted(check_mixture_cell(engine, lambda a: dev(a, engine), ZS_CELL, zs=True)) == ["mixture_zs", "mixture_zs_cov"]


def padded(a, ld, engine):
    """``a`` (rows x d) in a rows x ld device array with NaN in the padding columns."""
    out = np.full((a.shape[0], ld), np.nan)
    out[:, :a.shape[1]] = a
    return dev(out, engine)


def test_leading_dimensions_larger_than_d(engine):
    """One sgp_ctx_mixture_predict and one sgp_predict through the C ABI with ldx = d + 2, ldxs = d + 3, ldz = d + 1 and NaN in the
    padding columns: bit for bit the contiguous calls, so nothing of the padding reaches any output."""
    name = ZS_CELL
    inp, Xs = R.stream_inputs(name), R.stream_points(name)
    (N, d), M, T, S = inp["X"].shape, inp["Z"].shape[0], Xs.shape[0], 3
    draws = [R.draw(name, k) for k in range(S)]
    X, y, Xsd, Z = dev(inp["X"], engine), dev(inp["y"], engine), dev(Xs, engine), dev(inp["Z"], engine)
    Xp, Xsp, Zp = padded(inp["X"], d + 2, engine), padded(Xs, d + 3, engine), padded(inp["Z"], d + 1, engine)
    p_ = engine._ptr
    # --- the mixture route
    want = engine.mixture_predict(X, y, Xsd, Z, [dk[1].tolist() for dk in draws], [dk[2] for dk in draws], [dk[3] for dk in draws],
                                  jitter=inp["jitter"], kernel=inp["kernel"], full_cov=True, gate_jitter=GATE_JITTER)
    mean, var, cov = engine.empty(S, T), engine.empty(S, T), engine.empty(S, T, T)
    info, gate = (torch.full((S,), -99, dtype=torch.int32, device=engine.device) for _ in range(2))
    nbytes = engine.lib.sgp_mixture_predict_workspace_bytes(N, T, M, d, S, 1, 1)
    ws = engine._workspace("mixture", nbytes)
    inv = (C.c_double * (S * d))(*[1.0 / v for dk in draws for v in dk[1]])
    sf2c, s2c = (C.c_double * S)(*[dk[2] for dk in draws]), (C.c_double * S)(*[dk[3] for dk in draws])
    st = engine.lib.sgp_ctx_mixture_predict(engine._c(), p_(Xp), d + 2, p_(y), N, p_(Xsp), d + 3, T, p_(Zp), d + 1, S, inv, sf2c, s2c,
                                            float(inp["jitter"]), M, d, 0, 1, GATE_JITTER, p_(mean), p_(var), p_(cov),
                                            C.c_void_p(info.data_ptr()), C.c_void_p(gate.data_ptr()), p_(ws), ws.numel(), engine._stream())
    assert st == 0 and info.cpu().tolist() == [0] * S == gate.cpu().tolist() == want["info"].cpu().tolist()
    assert same_bits(mean, want["mean"]) and same_bits(var, want["var"]) and same_bits(cov, want["cov"])
    assert bool(mean.isfinite().all()) and bool(cov.isfinite().all())
    # --- sgp_predict from the factors of the whitened form
    import ggp_amd
    cb = ggp_amd.CollapsedBound(X, y, kernel=inp["kernel"], jitter=inp["jitter"], engine=engine, form="whitened")
    _, ls, sf2, s2 = draws[0]
    factors = cb.factors(Z, ls.tolist(), sf2, s2)
    wmean, wvar, wcov = cb.predict(Xsd, Z, ls.tolist(), sf2, s2, full_cov=True, factors=factors)
    mean, var, cov = engine.empty(T), engine.empty(T), engine.empty(T, T)
    ws = engine._workspace("predict", engine.lib.sgp_predict_workspace_bytes(T, M, d, 1))
    st = engine._cf.sgp_predict(p_(Xsp), d + 3, T, p_(Zp), d + 1, engine._inv_ls(ls.tolist(), d, inp["kernel"]), float(sf2), float(s2),
                                p_(factors), M, d, 0, 1, p_(mean), p_(var), p_(cov), p_(ws), ws.numel(), engine._stream())
    assert st == 0
    assert same_bits(mean, wmean) and same_bits(var, wvar) and same_bits(cov, wcov) and bool(cov.isfinite().all())
