"""CPU: the streaming posterior predictive -- sgp_predict from the ``factors`` of CollapsedBound (whitened and streaming form),
sgp_mixture_predict and sgp_mixture_predict_zs -- held to the long-double reference tests/vfe_predict_reference.py (its second half:
STREAM_CELLS, the full covariance, composite kernels, the float64 level of the route through unwhitened statistics).

Here, without a device: the caps on the tolerance at every cell from the reference alone, the deliberate defects failing the comparison
at named cells, and the ``check_*`` functions run on tests/fake_engine.py.  tests/test_stream_predict_gpu.py runs the same ``check_*``
functions on the device.

The rule is the family's: component-wise |got - ref| <= tol S, tol = 10 max(e64, 1e-13), e64 measured from float64 runs of the reference
(``stream_e64``), S the condition scale of the component.  Every check prints one line per cell and route with the worst |got - ref| / S
of each output next to its tolerance, and returns them ({route: {key: (worst, tol)}}: tools/stream_predict_ratios.py records them)."""
import numpy as np
import pytest
import torch

import vfe_predict_reference as R
import vfe_reference as V
from fake_engine import FactoredOracleEngine

import ggp_amd
from ggp_amd.core import TIER_STREAMING, TIER_WHITENED

GATE_JITTER = 1e-4                                          # the reference's PSD gate, cholesky(cov + 1e-4 I)
ZS_CELL = "300-65-2-rbf"                                    # sgp_mixture_predict_zs: Z_k = Z + 0.01 k noise_k
NOISE_FREE = ("300-65-2-rbf", "200-64-2-matern52")          # sgp_predict also with pred_noise = False: row 1 sits on an inducing input
_host = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))  # noqa: E731  (a copy: the cells' arrays are read-only)


def np64(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(np64(a)), np.ascontiguousarray(np64(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- shared checks
def judge(what, got, ref, S, tol, cap, strict=True):
    """Prints the worst |got - ref| / S of every key beside its tolerance, then asserts (``strict=False``: the measuring tool only wants
    the figures).  The cap on the tolerance is asserted either way: the rule must not hide a failure.  Returns {key: (worst, tol)}."""
    keys = tuple(k for k in R.COV_KEYS if k in got)
    assert all(R.tolerance(0.0) <= tol[k] and (cap is None or tol[k] <= cap) for k in keys), (what, tol, cap)
    w = R.worst(got, ref, S, keys)
    print("STREAM_PREDICT %s  %s" % (what, "  ".join("%s %.2g/%.1e" % (k, w[k], tol[k]) for k in keys)))
    bad = {k: (w[k], tol[k]) for k in keys if not w[k] <= tol[k]}
    assert not (bad and strict), (what, bad)
    return {k: (w[k], tol[k]) for k in keys}


def check_shape_properties(name, got, S, tol, pred_noise, k=0, zs=False, T=None):
    """What holds of any correct predictive at draw k of the cell: var = diag(cov) within the two tolerances, and at the far point
    100 * 1 of a stationary kernel the prior variance exactly (|a*|^2 lies below an ulp of it), and a mean of exactly zero where k_u*
    underflows to zero (``far_is_zero``: the RBF cells, but for the longest lengthscales of the ``ill`` ones)."""
    if "cov" in got:
        assert np.all(np.abs(np.diagonal(got["cov"]) - got["var"]) <= float(tol["var"] + tol["cov"]) * np.asarray(S["var"], np.float64)), name
    if name in R.STREAM_COMPOSITE:
        return
    _, _, sf2, s2 = R.draw(name, k, zs)
    for r in R.far_rows(name, T):
        assert got["var"][r] == sf2 + (s2 if pred_noise else 0.0), (name, r, got["var"][r])
        if R.far_is_zero(name, k, zs):
            assert got["mean"][r] == 0.0, (name, r, got["mean"][r])


def bound_of(engine, conv, name, form):
    inp = R.stream_inputs(name)
    cb = ggp_amd.CollapsedBound(conv(inp["X"]), conv(inp["y"]), kernel=inp["kernel"], jitter=inp["jitter"], engine=engine, form=form)
    Z, hyp, sf2, s2 = R.draw(name)
    Zd, hyp = conv(Z), [float(v) for v in hyp]
    factors = cb.factors(Zd, hyp, sf2, s2)
    assert cb.last_tier == (TIER_WHITENED if form == "whitened" else TIER_STREAMING)   # the route under test is the one that ran
    return cb, Zd, hyp, sf2, s2, factors


def check_predict_cell(engine, conv, name, form, strict=True):
    """sgp_predict at one cell from the ``factors`` of ``CollapsedBound(form=form)``: mean, var and the full covariance with the noise
    (and, at the NOISE_FREE cells, without), the covariance symmetric bit for bit."""
    cb, Zd, hyp, sf2, s2, factors = bound_of(engine, conv, name, form)
    Xs = conv(R.stream_points(name))
    out = {}
    for pred_noise in (True, False) if name in NOISE_FREE else (True,):
        mean, var, cov = cb.predict(Xs, Zd, hyp, sf2, s2, pred_noise=pred_noise, full_cov=True, factors=factors)
        T = Xs.shape[0]
        assert tuple(mean.shape) == tuple(var.shape) == (T,) and tuple(cov.shape) == (T, T)
        got = {"mean": np64(mean), "var": np64(var), "cov": np64(cov)}
        ref, S = R.stream_reference(name, 0, False, pred_noise)
        tol = R.stream_tolerances(name, form, 0, False, pred_noise)
        route = "predict_%s%s" % (form, "" if pred_noise else "_noise_free")
        out[route] = judge("%s %s" % (name, route), got, ref, S, tol, R.stream_cap(name, form), strict)
        assert same_bits(cov, cov.T.contiguous()), (name, route)   # the kernel symmetrises
        if strict:
            check_shape_properties(name, got, S, tol, pred_noise)
        mean2, var2, none = cb.predict(Xs, Zd, hyp, sf2, s2, pred_noise=pred_noise, factors=factors)
        assert none is None and same_bits(mean2, mean) and same_bits(var2, var)
    return out


def check_predict_big_t(engine, conv, form, bits, strict=True):
    """sgp_predict past its test-row chunk (16384 without a covariance) and at the mixture route's (8192): mean and var at every row --
    the last chunk is the far point alone -- and, with ``bits``, the leading 64 rows of the longest call bit for bit those of a
    64-row call."""
    name = R.BIG_T_CELL
    cb, Zd, hyp, sf2, s2, factors = bound_of(engine, conv, name, form)
    out = {}
    for T in R.BIG_T:
        Xs = conv(R.stream_points(name, T))
        mean, var, cov = cb.predict(Xs, Zd, hyp, sf2, s2, factors=factors)
        assert cov is None and tuple(mean.shape) == tuple(var.shape) == (T,)
        got = {"mean": np64(mean), "var": np64(var)}
        ref, S = R.stream_reference(name, 0, False, True, T)
        tol = R.stream_tolerances(name, form, 0, False, True, T)
        route = "predict_%s_T%d" % (form, T)
        out[route] = judge("%s %s" % (name, route), got, ref, S, tol, R.stream_cap(name, form), strict)
        if strict:
            check_shape_properties(name, got, S, tol, True, T=T)
    m64, v64, _ = cb.predict(Xs[:64].contiguous(), Zd, hyp, sf2, s2, factors=factors)
    judge("%s %s rows 0..63 alone" % (name, route), {"mean": np64(m64), "var": np64(v64)}, *({k: v[:64] for k, v in dct.items()} for dct in (ref, S)),
          tol, R.stream_cap(name, form), strict)
    if bits:
        assert same_bits(m64, mean[:64]) and same_bits(v64, var[:64])
    return out


def check_mixture_cell(engine, conv, name, zs=False, T=None, strict=True):
    """sgp_mixture_predict (``zs``: sgp_mixture_predict_zs) at the DRAWS = 9 draws of one cell -- two batches of MIXTURE_BATCH --, every
    draw against the reference at its own theta_k (and Z_k): with the full covariance and the PSD gate, and without; ``info`` and
    ``gate`` zero, the covariance symmetric within its tolerance, mean and var of the two modes the same bits."""
    inp = R.stream_inputs(name)
    draws = [R.draw(name, k, zs) for k in range(R.DRAWS)]
    Xs = R.stream_points(name, T)
    full = R.with_cov(Xs.shape[0])
    Z = conv(np.stack([dk[0] for dk in draws])) if zs else conv(inp["Z"])
    args = (conv(inp["X"]), conv(inp["y"]), conv(Xs), Z, [dk[1].tolist() for dk in draws], [dk[2] for dk in draws], [dk[3] for dk in draws])
    kw = dict(jitter=inp["jitter"], kernel=inp["kernel"], pred_noise=True)
    r = engine.mixture_predict(*args, **kw)
    assert r["cov"] is None and r["gate"] is None and np64(r["info"]).tolist() == [0] * R.DRAWS
    runs = {"mixture%s" % ("_zs" if zs else ""): r}
    if full:
        rc = engine.mixture_predict(*args, full_cov=True, gate_jitter=GATE_JITTER, **kw)
        assert np64(rc["info"]).tolist() == [0] * R.DRAWS and np64(rc["gate"]).tolist() == [0] * R.DRAWS
        assert same_bits(rc["mean"], r["mean"]) and same_bits(rc["var"], r["var"])
        runs["mixture%s_cov" % ("_zs" if zs else "")] = rc
    out = {}
    for route, res in runs.items():
        for k in range(R.DRAWS):
            got = {key: np64(res[key])[k] for key in (R.COV_KEYS if res["cov"] is not None else R.KEYS)}
            ref, S = R.stream_reference(name, k, zs, True, T)
            tol = R.stream_tolerances(name, "whitened", k, zs, True, T)
            w = judge("%s %s draw %d" % (name, route, k), got, ref, S, tol, R.draw_cap(name, k), strict)
            for key, (wk, tk) in w.items():
                if key not in out.setdefault(route, {}) or wk / tk > out[route][key][0] / out[route][key][1]:
                    out[route][key] = (wk, tk)
            if "cov" in got:
                asym = np.abs(got["cov"] - got["cov"].T)
                assert not strict or np.all(asym <= float(tol["cov"]) * np.asarray(S["cov"], np.float64)), (name, route, k, asym.max())
            if strict:
                check_shape_properties(name, got, S, tol, True, k, zs, T)
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name", list(R.STREAM_CELLS) + [R.BIG_T_CELL + "-T%d" % T for T in R.BIG_T])
def test_the_tolerance_rule_cannot_hide_a_failure(name):
    """tol = 10 max(e64, 1e-13) from the reference alone: at or below 1e-10 on the whitened routes of an untagged cell, 1e-8 at the ``ill``
    cells, 1e-7 on the streaming form (not run at the ``ill`` cells) -- every output, with and without the noise; and the long-double
    reference itself has the shape properties the device is asked for."""
    name, T = (R.BIG_T_CELL, int(name.rsplit("-T", 1)[1])) if "-T" in name else (name, None)
    for route in R.ROUTES:
        if name not in R.stream_cells(route):
            assert name in R.STREAM_ILL and route == "streaming"
            continue
        for pred_noise in (True, False):
            tol = R.stream_tolerances(name, route, 0, False, pred_noise, T)
            assert tuple(tol) == R.stream_keys(name, T)
            assert all(1e-12 <= tol[k] <= R.stream_cap(name, route) for k in tol), (name, route, pred_noise, tol)
            ref, S = R.stream_reference(name, 0, False, pred_noise, T)
            check_shape_properties(name, {k: np.asarray(v, np.float64) for k, v in ref.items()}, S, tol, pred_noise, T=T)
    assert [n for n in R.STREAM_STATIONARY if not R.far_is_zero(n)] == ["200-64-2-matern52", "400-257-3-matern32", "8193-5-1-matern32"]   # every RBF cell
    assert R.CAP_STREAMING == 1e-7 and (R.CAP_UNTAGGED, R.CAP_TAGGED) == (1e-10, 1e-8) and (V.MARGIN, V.FLOOR) == (10, 1e-13)


def test_the_draws_tolerances_are_capped_too():
    """Draw k > 0 of an untagged cell stays at or below 1e-8 (the per-sample inducing inputs included); at the ``ill`` cells exactly the
    draws of LOOSE_DRAWS lie beyond it, where the two float64 orders themselves disagree with long double by more than 1e-9 of the scale."""
    loose = {}
    for name in R.STREAM_STATIONARY:
        for zs in (False, True) if name == ZS_CELL else (False,):
            for k in range(1, R.DRAWS):
                tol = R.stream_tolerances(name, "whitened", k, zs)
                if name in R.STREAM_ILL:
                    if max(tol.values()) > R.CAP_TAGGED:
                        loose.setdefault(name, []).append(k)
                else:
                    assert R.draw_cap(name, k) == R.CAP_TAGGED and max(tol.values()) <= R.CAP_TAGGED, (name, zs, k, tol)
    assert {n: tuple(v) for n, v in loose.items()} == R.LOOSE_DRAWS
    tol = [R.stream_tolerances(R.BIG_T_CELL, "whitened", k, False, True, R.BIG_T[0]) for k in range(R.DRAWS)]
    assert max(max(t.values()) for t in tol) <= R.CAP_UNTAGGED


def test_the_streaming_level_is_the_worse_of_its_two_orders():
    """``measure_e64_streaming`` is the worse of oracle.predict as it is and the explicit-inverse sandwich, per key; at a cell whose K_uu
    is not trivial it lies well above the whitened level -- the reason the streaming form has a tolerance of its own."""
    name = "300-65-2-rbf"
    ref, S = R.stream_reference(name)
    each = [R.worst(R.streaming64(name, order), ref, S, R.COV_KEYS) for order in ("oracle", "sandwich")]
    e = R.measure_e64_streaming(name)
    assert e == {k: max(each[0][k], each[1][k]) for k in R.COV_KEYS}
    white = R.stream_e64(name, "whitened")
    assert all(e[k] > 10 * white[k] for k in R.COV_KEYS), (e, white)


# mutation -> (the cells it must be caught at, the output that catches it)
CAUGHT = {
    "no_v2": (("300-65-2-rbf", "400-257-3-matern32", "200-65-1-composite-co2"), "var"),
    "no_jitter": (("300-65-2-rbf", "8193-5-1-matern32"), "var"),
    "no_noise": (("50-5-1-rbf", "300-129-3-rbf"), "var"),
    "cov_no_ctc": (("300-65-2-rbf", "130-130-3-rbf", "130-17-1-composite-co2"), "cov"),
    "cov_noise_everywhere": (("200-64-2-matern52", "8193-5-1-matern32", "200-64-2-rbf-ill"), "cov"),
    "cov_kss_diag": (("1-1-1-rbf", "300-129-3-rbf", "200-65-1-composite-co2"), "cov"),
    "cov_row_shift": (("300-65-2-rbf", "130-130-3-rbf", "400-257-3-matern32"), "cov"),
    "mean_wrong_s2": (("200-64-2-matern52", "300-65-2-rbf", "8193-5-1-matern32"), "mean"),
}


@pytest.mark.parametrize("mutate", R.MUTATIONS + R.COV_MUTATIONS)
def test_deliberate_defects_fail_the_comparison(mutate):
    """Every defect is caught at its named cells under the tolerance of BOTH routes (the streaming form's is the wider one)."""
    cells, key = CAUGHT[mutate]
    for name in cells:
        ref, S = R.stream_reference(name)
        bad = R.stream_evaluate(name, mutate=mutate)[0]
        w = R.worst(bad, ref, S, R.COV_KEYS)
        for route in R.ROUTES:
            if name in R.stream_cells(route):
                tol = R.stream_tolerances(name, route)
                assert w[key] > tol[key], (mutate, name, route, w, tol)
                with pytest.raises(AssertionError):
                    judge("%s %s" % (name, mutate), bad, ref, S, tol, R.stream_cap(name, route))
    assert set(CAUGHT) == set(R.MUTATIONS + R.COV_MUTATIONS)


def test_a_shifted_row_in_the_last_chunk_is_caught_at_the_big_t_cell():
    """The one-row last chunk of the T = 8193 / 16385 calls: a defect there (the far point answered with its neighbour's column) fails
    mean and var of that row alone."""
    name = R.BIG_T_CELL
    for T in R.BIG_T:
        ref, S = R.stream_reference(name, 0, False, True, T)
        bad = R.stream_evaluate(name, T=T, mutate="cov_row_shift")[0]
        for route in R.ROUTES:
            tol = R.stream_tolerances(name, route, 0, False, True, T)
            err = np.abs(np.asarray(bad["var"] - ref["var"], np.float64)) / np.asarray(S["var"], np.float64)
            assert err[T - 1] > tol["var"] and np.all(err[:T - 1] == 0.0), (T, route, err[T - 1])


# ---------------------------------------------------------------------------------------------------------------- the routes on the CPU
@pytest.mark.parametrize("name,form", [(n, f) for f in R.ROUTES for n in R.stream_cells(f) if n in R.STREAM_STATIONARY])
def test_fake_engine_predict_meets_the_bound(name, form):
    check_predict_cell(FactoredOracleEngine(), _host, name, form)


@pytest.mark.parametrize("form", R.ROUTES)
def test_fake_engine_predict_past_the_test_row_chunks(form):
    check_predict_big_t(FactoredOracleEngine(), _host, form, bits=False)


@pytest.mark.parametrize("name", R.STREAM_STATIONARY)
def test_fake_engine_mixture_meets_the_bound(name):
    eng = FactoredOracleEngine()
    out = check_mixture_cell(eng, _host, name)
    assert sorted(out) == ["mixture", "mixture_cov"] and eng.calls["mixture_predict"] == 2


def test_fake_engine_mixture_with_inducing_inputs_per_draw_and_past_the_chunk():
    eng = FactoredOracleEngine()
    assert sorted(check_mixture_cell(eng, _host, ZS_CELL, zs=True)) == ["mixture_zs", "mixture_zs_cov"]
    assert sorted(check_mixture_cell(eng, _host, R.BIG_T_CELL, T=R.BIG_T[0])) == ["mixture"]
    # a draw's own Z reached the reference: judged against the shared Z it fails
    inp, name = R.stream_inputs(ZS_CELL), ZS_CELL
    draws = [R.draw(name, k, True) for k in range(R.DRAWS)]
    r = eng.mixture_predict(_host(inp["X"]), _host(inp["y"]), _host(R.stream_points(name)), _host(np.stack([dk[0] for dk in draws])),
                            [dk[1].tolist() for dk in draws], [dk[2] for dk in draws], [dk[3] for dk in draws], jitter=inp["jitter"])
    ref, S = R.stream_reference(name, 8, False)
    with pytest.raises(AssertionError):
        judge("shared Z", {"mean": np64(r["mean"])[8], "var": np64(r["var"])[8]}, ref, S, R.stream_tolerances(name, "whitened", 8), R.CAP_UNTAGGED)
    with pytest.raises(ValueError):
        eng.mixture_predict(_host(inp["X"]), _host(inp["y"]), _host(R.stream_points(name)), _host(np.stack([dk[0] for dk in draws[:3]])),
                            [dk[1].tolist() for dk in draws], [dk[2] for dk in draws], [dk[3] for dk in draws])
