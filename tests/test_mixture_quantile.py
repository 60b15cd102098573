"""CPU: the mixture quantiles around their kernel -- the ABI of libsgp_mixture_hip.so and its registration, the host-side refusals, the
acceptance rule of tests/mixture_quantile_reference.py on the plain-C++ arithmetic of csrc/sgp_mixture.hpp (a stand-alone host program
under AddressSanitizer + UBSan, with an 80-bit restatement beside it as the control that the rule is satisfiable) and on the CPU doubles
(tests/mixture_quantile_double.py), that the rule discriminates, and the public layer on those doubles: ``probs=`` on the batched
predictives and the results' ``predict``, ``interval`` / ``coverage`` / ``interval_width``, ``ggp_amd.mixture_quantiles`` and the
experiment's ``--calibration``."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mixture_quantile_reference as R
from conftest import ROOT
from mixture_quantile_double import ExactQuantileDouble, SgprQuantileDouble, quantiles_numpy

import ggp_amd
import ggp_amd._lib as L

CSRC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
NAMES = {"sgp_mixture_quantiles_workspace_bytes": 3, "sgp_mixture_quantiles": 15, "sgp_ctx_mixture_quantiles": 16}
ENTRY = ("libsgp_mixture_hip.so", ["sgp_mixture.hip"], "sgp_mixture.h")
FIVE = [("libsgp_exact_nuts_hip.so", ["sgp_exact_nuts.hip"], "sgp_exact_nuts.h"),
        ("libsgp_exact_predict_hip.so", ["sgp_exact_predict.hip"], "sgp_exact_predict.h"),
        ("libsgp_vfe_batch_hip.so", ["sgp_vfe_batch.hip"], "sgp_vfe_batch.h"),
        ("libsgp_vfe_nuts_hip.so", ["sgp_vfe_nuts.hip"], "sgp_vfe_nuts.h"),
        ("libsgp_vfe_predict_hip.so", ["sgp_vfe_predict.hip"], "sgp_vfe_predict.h")]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load_mixture_library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    """include/sgp_mixture.h = the dynamic symbol table of libsgp_mixture_hip.so = MIXTURE_PROTOTYPES; all it takes from the core is
    sgp_ctx_device; the core's surface and the first five companions are what they were."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp_mixture.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sgp_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(L.MIXTURE_PROTOTYPES)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.MIXTURE_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", L.MIXTURE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(NAMES)
    und = subprocess.run([nm, "-D", "--undefined-only", L.MIXTURE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert [ln.split()[-1] for ln in und.splitlines() if re.search(r"\bsgp_", ln)] == ["sgp_ctx_device"]
    core = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert "sgp_mixture_quantiles" not in core and L.SGP_ABI_VERSION == 3 and len(L.PROTOTYPES) == 146
    for table in (L.PROTOTYPES, L.EXACT_NUTS_PROTOTYPES, L.EXACT_PREDICT_PROTOTYPES, L.VFE_BATCH_PROTOTYPES, L.VFE_NUTS_PROTOTYPES,
                  L.VFE_PREDICT_PROTOTYPES):
        assert not any(n in table for n in NAMES)
    assert L._COMPANION_TABLE["mixture"] == (L.MIXTURE_LIB_PATH, L.MIXTURE_PROTOTYPES)
    assert (L.MIXTURE_MAX_Q, L.MIXTURE_P_MIN) == (R.K["MAXQ"], R.K["PMIN"]) == (8, 1e-9)
    assert hasattr(ggp_amd.HipEngine, "mixture_quantiles") and hasattr(ggp_amd.HipEngine, "mixture_lib")
    import ggp_amd.build as B
    assert B.COMPANIONS == FIVE and B.COMPANIONS_MORE == [ENTRY] and "sgp_mixture.hip" not in B.SOURCES
    # the constants the header quotes are the .hpp's, and the measured erfc error is the profile's
    head = open(os.path.join(ROOT, "include", "sgp_mixture.h")).read()
    prof = json.load(open(os.path.join(ROOT, "profiles", "mixture_quantile_erfc_ulp.json")))
    assert prof["worst_ulp"] == R.K["ERFC_ULP"] and prof["points"] == 100000 and prof["range"] == [-9.0, 9.0]
    assert "MQ_C = 2 x %s + 4 = %.4f" % (R.K["ERFC_ULP"], R.K["C"]) in head and "MQ_MAX_ITERS = %d" % R.K["MAX_ITERS"] in head
    assert R.K["WIDTH"] == 2.0 ** -48 and "2^-48 (|x| + sigma_min)" in head


def test_the_digest_covers_the_new_library(lib, tmp_path, monkeypatch):
    """build() reuses the library while its digest is unchanged: its source, its header and every csrc header are in it."""
    spec = importlib.util.spec_from_file_location("_sgp_build_mq", os.path.join(ROOT, "generalised-gaussian-processes_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    (name, sources, header), = b.COMPANIONS_MORE
    before = b._companion_digest(b._digest(), sources, header)
    assert before == open(os.path.join(b.CSRC, name + ".sha256")).read().strip()
    work = tmp_path / "pkg" / "csrc"
    work.mkdir(parents=True)
    for f in os.listdir(b.CSRC):
        if f.endswith((".hip", ".hpp", ".map")):
            shutil.copy(os.path.join(b.CSRC, f), work / f)
    (tmp_path / "include").mkdir()
    for h in ("sgp.h", header):
        shutil.copy(os.path.join(ROOT, "include", h), tmp_path / "include" / h)
    monkeypatch.setattr(b, "CSRC", str(work))
    assert b._companion_digest(b._digest(), sources, header) == before
    for edited in (work / "sgp_mixture.hip", work / "sgp_mixture.hpp", work / "sgp_wg_dense.hpp", work / "sgp_common.hpp",
                   tmp_path / "include" / header):
        with open(edited, "a") as fh:
            fh.write("// a comment\n")
        after = b._companion_digest(b._digest(), sources, header)
        assert after != before, edited
        before = after


# ---------------------------------------------------------------------------------------------------------------- refusals, no device
def _args(**bad):
    a = dict(mean=8, var=8, info=8, off=8, G=3, T=7, probs=(0.025, 0.975), Q=None, Y=8, quant=8, pit=8, iters=8, ws=8, nbytes=256)
    a.update(bad)
    p = lambda k: C.c_void_p(a[k])  # noqa: E731  (the dummy 8 is never dereferenced: every call here fails validation first)
    pr = None if a["probs"] is None else (C.c_double * len(a["probs"]))(*a["probs"])
    Q = a["Q"] if a["Q"] is not None else (len(a["probs"]) if a["probs"] is not None else 1)
    return (p("mean"), p("var"), p("info"), p("off"), a["G"], a["T"], pr, Q, p("Y"), p("quant"), p("pit"), p("iters"), p("ws"),
            a["nbytes"], None)


NINE = tuple(0.1 * k for k in range(1, 10))
ROWS = [  # (what is wrong, status): SGP_ERR_ARG = -1 before SGP_ERR_DIM = -2 before SGP_ERR_WORKSPACE = -3, all before any launch
    (dict(G=2 ** 24), -2), (dict(T=32769), -2), (dict(G=0), -1), (dict(T=0), -1), (dict(Q=0), -1), (dict(probs=NINE), -1),
    (dict(probs=NINE, Q=9), -1), (dict(probs=(0.5, 9e-10)), -1), (dict(probs=(1.0,)), -1), (dict(probs=(0.0,)), -1),
    (dict(probs=(float("nan"),)), -1), (dict(probs=(-0.5,)), -1), (dict(probs=(1.0 - 1e-10,)), -1), (dict(probs=None), -1),
    (dict(mean=0), -1), (dict(var=0), -1), (dict(info=0), -1), (dict(off=0), -1), (dict(quant=0), -1), (dict(pit=0), -1),
    (dict(ws=0), -3), (dict(nbytes=255), -3), (dict(T=32769, probs=(2.0,)), -1), (dict(G=2 ** 24, quant=0), -1), (dict(T=32769, ws=0), -2),
]


def test_out_of_range_arguments_are_refused_on_the_host(lib):
    for bad, want in ROWS:
        assert lib.sgp_mixture_quantiles(*_args(**bad)) == want, bad
        assert lib.sgp_ctx_mixture_quantiles(None, *_args(**bad)) == want, bad
    q = lib.sgp_mixture_quantiles_workspace_bytes
    assert q(1, 1, 1) == 256 == q(2 ** 24 - 1, 32768, 8)
    for shape in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 9), (2 ** 24, 1, 1), (1, 32769, 1)]:
        assert q(*shape) == 0, shape
    # the engine's own intake, before it allocates: it runs on CPU tensors
    cpu = torch.device("cpu")
    intake = ggp_amd.HipEngine._mixture_quantiles_intake
    m, v, i = torch.zeros(6, 4, dtype=torch.float64), torch.ones(6, 4, dtype=torch.float64), torch.zeros(6, dtype=torch.int32)
    P, T, G, off, pr = intake(cpu, m, v, i, [0, 2, 2, 6], (0.025, 0.975), torch.zeros(3, 4, dtype=torch.float64))
    assert (P, T, G, off.tolist(), list(pr)) == (6, 4, 3, [0, 2, 2, 6], [0.025, 0.975])
    for bad in (dict(probs=()), dict(probs=NINE), dict(probs=(0.5, 1e-10)), dict(probs=(float("nan"),)), dict(offsets=[0, 3]),
                dict(offsets=[1, 6]), dict(offsets=[0, 4, 2, 6]), dict(offsets=[0.0, 6.0]), dict(offsets=[6]), dict(mean=m.float()),
                dict(var=v[:5]), dict(info=i.long()), dict(info=i[:5]), dict(info=i.numpy()), dict(mean=m.t()),
                dict(Ytest=torch.zeros(3, 5, dtype=torch.float64)), dict(Ytest=torch.zeros(3, 4))):
        kw = dict(mean=m, var=v, info=i, offsets=[0, 2, 2, 6], probs=(0.5,), Ytest=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            intake(cpu, **kw)


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def _case_text(mean, var, info, off, probs, Y):
    G, (P, T) = len(off) - 1, mean.shape
    rows = ["%d %d %d %d %d" % (G, T, P, len(probs), 1), " ".join(float(p).hex() for p in probs), " ".join(map(str, off.tolist())),
            " ".join(str(int(k)) for k in info)]
    rows += [" ".join(float(x).hex() for x in a.reshape(-1)) for a in (mean, var, Y)]
    return "\n".join(rows) + "\n"


def test_the_arithmetic_on_the_host_under_asan_ubsan_meets_the_acceptance_rule(tmp_path):
    """tests/native/mixture_quantile_host.cpp (its own main, csrc/sgp_mixture.hpp alone) on every family x the five probabilities, an
    empty group and a group with failed draws: mq_point's quantiles meet the acceptance rule, its pit the derived bound, its iteration
    count the cap; the 80-bit bisection beside it meets the rule too (the rule is satisfiable); a draw with v = 0, v < 0 or a NaN
    makes its test point NaN and changes no bit of the others."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on CPU-only hosts, never on a GPU box")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "mixture_quantile_host_asan")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-I", CSRC, "-o", exe,
                                                                           os.path.join(ROOT, "tests", "native", "mixture_quantile_host.cpp")],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    T = 4
    mean, var, info, off, Y, names = R.batch(T)
    G, Q = len(names), len(R.PROBS)
    m0, v0 = np.nan_to_num(mean, nan=0.0), np.nan_to_num(var, nan=1.0)  # (the failed draws' rows are never read)

    def run(m, v, probs, tag):
        case = tmp_path / (tag + ".txt")
        case.write_text(_case_text(m, v, info, off, probs, Y))
        r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "mixture quantile host ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
        rows = [w for w in map(str.split, r.stdout.splitlines()[:-1])]
        nq = len(probs)
        got = np.array([[float.fromhex(x) for x in w[3:]] for w in rows]).reshape(G, T, 1 + 2 * nq)
        iters = np.array([int(w[2]) for w in rows]).reshape(G, T)
        return (np.ascontiguousarray(got[:, :, 1:1 + nq].transpose(0, 2, 1)), np.ascontiguousarray(got[:, :, 1 + nq:].transpose(0, 2, 1)),
                np.ascontiguousarray(got[:, :, 0]), iters)
    quant, ctrl, pit, iters = run(m0, v0, R.PROBS, "families")
    cols = list(range(T))
    worst = R.check_batch(quant, pit, iters, R.PROBS, mean, var, info, off, Y, names, columns=cols)
    R.check_batch(ctrl, None, None, R.PROBS, mean, var, info, off, Y, names, columns=cols)   # the control: the rule is satisfiable
    print("host arithmetic: worst", worst, "iterations per family", dict(zip(names, iters.max(1).tolist())))
    assert worst["max_iters"] < 100   # the safeguarded Newton step must do better than the cap by far
    g1 = names.index("single")  # S = 1, mu = 3, sigma = 2: mu + sigma Phi^-1(p), Phi^-1(0.975) = 1.959963984540054...
    assert abs(quant[g1, 3, 0] - (3.0 + 2.0 * 1.959963984540054)) < 1e-13 and abs(quant[g1, 2, 0] - 3.0) < 1e-13
    # Q = 1 and Q = 2 (other instantiations, other neighbours): the same bits
    for probs, qs in (((0.975,), [3]), ((0.025, 0.975), [1, 3])):
        q_, _, pit_, _ = run(m0, v0, probs, "q%d" % len(probs))
        assert np.array_equal(q_.view(np.uint64), quant[:, qs].view(np.uint64)) and np.array_equal(pit_.view(np.uint64), pit.view(np.uint64))
    # degenerate draws: that test point alone
    gm, gs = names.index("many"), names.index("scales")
    m1, v1 = m0.copy(), v0.copy()
    v1[off[gm] + 5, 1] = 0.0
    v1[off[gm] + 999, 2] = -1.0
    m1[off[gs], 3] = np.nan
    v1[off[names.index("identical")] + 1, 0] = np.inf
    q1, _, pit1, it1 = run(m1, v1, R.PROBS, "degenerate")
    hit = np.zeros((G, T), dtype=bool)
    hit[gm, 1] = hit[gm, 2] = hit[gs, 3] = hit[names.index("identical"), 0] = True
    assert np.isnan(q1.transpose(0, 2, 1)[hit]).all() and np.isnan(pit1[hit]).all() and (it1[hit] == 0).all()
    keep = ~hit
    assert np.array_equal(q1.transpose(0, 2, 1)[keep].view(np.uint64), quant.transpose(0, 2, 1)[keep].view(np.uint64))
    assert np.array_equal(pit1[keep].view(np.uint64), pit[keep].view(np.uint64))


def test_the_rule_discriminates_and_the_double_meets_it():
    """The numpy double meets the acceptance rule on every family; an answer moved by 1e-9 (|x| + sigma_min) fails it everywhere but at
    the median of the bimodal family, whose flat gap makes every x of it a correct answer."""
    mean, var, info, off, Y, names = R.batch(R.VARIANTS)
    quant, pit = quantiles_numpy(mean, var, info, off, R.PROBS, Y)
    R.check_batch(quant, pit, None, R.PROBS, mean, var, info, off, Y, names)
    rejected = 0
    for g, name in enumerate(names):
        if name == "empty":
            continue
        mu, sg = R.kept_moments(mean[off[g]:off[g + 1], 0], var[off[g]:off[g + 1], 0], info[off[g]:off[g + 1]])
        for q, p in enumerate(R.PROBS):
            x = float(quant[g, q, 0])
            for sign in (-1.0, 1.0):
                ok, fig = R.accept(x + sign * 1e-9 * (abs(x) + sg.min()), p, mu, sg)
                if name == "bimodal" and p == 0.5:
                    continue
                assert not ok, (name, p, sign, fig)
                rejected += 1
    assert rejected == 2 * (len(R.PROBS) * 8 - 1)
    assert 9.0 <= R.K["C"] <= 12.0 and R.K["MAX_ITERS"] == 256   # c = 2 x (an erfc of a few ulp) + 4; nothing here is tuned to a test


# ---------------------------------------------------------------------------------------------------------------- the public layer
def _toy(B=3, S=5, N=9, T=6, d=1, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (B, N, d))
    Y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, N))
    Xt = rng.uniform(-2.0, 2.0, (B, T, d))
    Yt = np.sin(Xt.sum(2)) + 0.1 * rng.standard_normal((B, T))
    q = rng.uniform(-0.5, 0.5, (B, S, d + 2))
    q[..., -1] -= 1.5
    return X, Y, Xt, Yt, q


def _check_fields(r, Yt, probs, B, T):
    assert r.probs.tolist() == list(probs) and r.quantiles.shape == (B, len(probs), T) and r.pit.shape == (B, T)
    want, pit = quantiles_numpy(r.draw_mean.reshape(-1, T), r.draw_var.reshape(-1, T), r.info.reshape(-1),
                                np.arange(B + 1) * r.draw_mean.shape[1], probs, Yt)
    assert np.array_equal(want, r.quantiles, equal_nan=True) and np.array_equal(pit, r.pit, equal_nan=True)
    lower, upper = r.interval(0.95)
    assert np.array_equal(lower, r.quantiles[:, 0]) and np.array_equal(upper, r.quantiles[:, -1]) and (lower < r.mean).all() and \
        (r.mean < upper).all()
    assert np.array_equal(r.interval_width(0.95), (upper - lower).mean(1)) and r.interval_width().shape == (B,)
    inside = ((Yt >= lower) & (Yt <= upper)).mean(1)
    assert np.array_equal(r.coverage(0.95), inside) and r.coverage().shape == (B,)
    with pytest.raises(ValueError, match="no quantile"):
        r.interval(0.9)
    with pytest.raises(ValueError, match="no quantile"):
        r.interval_width(0.5)
    assert r.coverage(0.5).shape == (B,)   # any level follows from the PIT


def test_probs_on_the_batched_predictives():
    X, Y, Xt, Yt, q = _toy()
    B, S, T = q.shape[0], q.shape[1], Xt.shape[1]
    probs = (0.025, 0.5, 0.975)
    eng = ExactQuantileDouble()
    plain = ggp_amd.predict_exact_batch(X, Y, q, Xt, Yt, engine=eng)
    assert eng.calls["mixture_quantiles"] == 0 and eng.calls["exact_mixture"] == 1
    assert plain.probs is None and plain.quantiles is None and plain.pit is None
    with pytest.raises(ValueError, match="no quantile"):
        plain.interval()
    with pytest.raises(ValueError, match="coverage needs"):
        plain.coverage()
    r = ggp_amd.predict_exact_batch(X, Y, q, Xt, Yt, engine=eng, probs=probs)
    assert eng.calls["mixture_quantiles"] == 1 and eng.calls["exact_mixture"] == 2 and eng.calls["exact_predict_batch"] == 2
    assert np.array_equal(r.mean, plain.mean) and np.array_equal(r.logpdf, plain.logpdf) and np.array_equal(r.draw_var, plain.draw_var)
    _check_fields(r, Yt, probs, B, T)
    no_y = ggp_amd.predict_exact_batch(X, Y, q, Xt, engine=eng, probs=probs)
    assert no_y.pit is None and np.array_equal(no_y.quantiles, r.quantiles)
    with pytest.raises(ValueError, match="coverage needs"):
        no_y.coverage()
    th = ggp_amd.exact_predict.constrain_samples(q)
    rt = ggp_amd.exact_predict.predict_theta_batch(X, Y, th, Xt, Yt, engine=eng, probs=probs)
    assert np.array_equal(rt.quantiles, r.quantiles) and np.array_equal(rt.pit, r.pit)
    for bad in ((), (0.5, 2.0), tuple(0.1 * k for k in range(1, 10))):
        with pytest.raises(ValueError, match="probs"):
            ggp_amd.predict_exact_batch(X, Y, q, Xt, Yt, engine=eng, probs=bad)
    # a draw that fails is left out of the quantiles as it is of the moments
    q2 = q.copy()
    q2[1, 2] = np.nan
    r2 = ggp_amd.predict_exact_batch(X, Y, q2, Xt, Yt, engine=eng, probs=probs)
    assert r2.kept.tolist() == [S, S - 1, S] and np.isfinite(r2.quantiles).all()
    assert np.array_equal(r2.quantiles[[0, 2]], r.quantiles[[0, 2]]) and not np.array_equal(r2.quantiles[1], r.quantiles[1])
    # the sparse twin
    Z = X[:, :4].copy()
    es = SgprQuantileDouble()
    sp0 = ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, Yt, engine=es)
    assert es.calls["mixture_quantiles"] == 0 and sp0.quantiles is None
    sp = ggp_amd.predict_sgpr_batch(X, Y, Z, q, Xt, Yt, engine=es, probs=probs)
    assert isinstance(sp, ggp_amd.SgprMixturePredictive) and es.calls["mixture_quantiles"] == 1 and es.calls["vfe_predict_batch"] == 2
    assert np.array_equal(sp.bound, sp0.bound) and np.array_equal(sp.logpdf, sp0.logpdf)
    _check_fields(sp, Yt, probs, B, T)
    spt = ggp_amd.sgpr_predict.predict_sgpr_theta_batch(X, Y, Z, ggp_amd.sgpr_predict.constrain_sgpr_samples(q), Xt, Yt, engine=es,
                                                        probs=probs)
    assert np.array_equal(spt.quantiles, sp.quantiles)


def test_results_pass_probs_on_and_the_host_moments_function():
    rng = np.random.default_rng(5)
    B, N, M = 2, 12, 4
    X = np.sort(rng.uniform(-3.0, 3.0, (N, 1)), 0)
    Y = np.sin(X[:, 0])[None] + 0.2 * rng.standard_normal((B, N))
    Z = X[np.round(np.linspace(0, N - 1, M)).astype(int)].copy()
    Xt, Yt = rng.uniform(-3.0, 3.0, (6, 1)), rng.standard_normal((B, 6))
    probs = (0.025, 0.975)
    eng = SgprQuantileDouble()
    post = ggp_amd.sample_exact_nuts_batch(X, Y, 6, 8, chains=2, seed=1, engine=eng)
    assert post.predict(Xt, Yt).quantiles is None and eng.calls["mixture_quantiles"] == 0
    r = post.predict(Xt, Yt, probs=probs)
    _check_fields(r, Yt, probs, B, 6)
    spost = ggp_amd.sample_sgpr_nuts_batch(X, Y, Z, 6, 8, chains=2, seed=1, jitter=1e-5, engine=eng)
    rs = spost.predict(Xt, Yt, thin=2, probs=probs)
    assert rs.draw_mean.shape == (B, 6, 6)
    _check_fields(rs, Yt, probs, B, 6)
    fit = ggp_amd.fit_ml2(X, Y, theta0=[1.0, 1.0, 0.1], bounds=np.array([(1e-2, 1e3), (1e-5, 1e5), (1e-5, 1e5)]), n_restarts=1, seed=0,
                          engine=eng, max_iter=3)
    p = fit.predict(Xt, Yt, probs=probs)
    _check_fields(p, Yt, probs, B, 6)
    # S = 1: the quantile of one Gaussian
    assert np.allclose(p.quantiles[:, 1], p.mean + 1.959963984540054 * np.sqrt(p.var), rtol=1e-13, atol=0)
    sfit = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=3, lr=0.05, seed=0, engine=eng)
    _check_fields(sfit.predict(Xt, Yt, probs=probs), Yt, probs, B, 6)
    n_calls = eng.calls["mixture_quantiles"]
    assert n_calls == 4
    # moments that are on the host: one call, B x S x T or S x T
    quant, pit = ggp_amd.mixture_quantiles(r.draw_mean, r.draw_var, probs, info=r.info, y=Yt, engine=eng)
    assert eng.calls["mixture_quantiles"] == n_calls + 1
    assert np.array_equal(quant, r.quantiles) and np.array_equal(pit, r.pit)
    q0, none = ggp_amd.mixture_quantiles(r.draw_mean[0], r.draw_var[0], probs, engine=eng)
    assert none is None and np.array_equal(q0, r.quantiles[0])
    q1, pit1 = ggp_amd.mixture_quantiles(r.draw_mean[1], r.draw_var[1], (0.975,), y=Yt[1], engine=eng)
    assert q1.shape == (1, 6) and np.array_equal(q1[0], r.quantiles[1, 1]) and np.array_equal(pit1, r.pit[1])
    info = np.zeros(r.info.shape, dtype=np.int32)
    info[0, 3] = 2
    qi, _ = ggp_amd.mixture_quantiles(r.draw_mean, r.draw_var, probs, info=info, engine=eng)
    assert np.array_equal(qi[1], r.quantiles[1]) and not np.array_equal(qi[0], r.quantiles[0])
    for bad in (dict(draw_var=r.draw_var[:, :3]), dict(info=np.zeros(5)), dict(y=Yt[:, :3]), dict(y=Yt[0]), dict(probs=(0.0,)),
                dict(draw_mean=r.draw_mean[0, 0], draw_var=r.draw_var[0, 0])):
        kw = dict(draw_mean=r.draw_mean, draw_var=r.draw_var, probs=probs, engine=eng)
        kw.update(bad)
        with pytest.raises(ValueError):
            ggp_amd.mixture_quantiles(**kw)
    # the host function of the parent commit on the same moments: the same 2.5 % / 97.5 % points, to its own bisection's accuracy
    lo, hi = ggp_amd.get_posterior_predictive_uncertainty_intervals(r.draw_mean[0], np.sqrt(r.draw_var[0]))
    assert np.allclose(lo, r.quantiles[0, 0], rtol=1e-9, atol=1e-9) and np.allclose(hi, r.quantiles[0, 1], rtol=1e-9, atol=1e-9)


def test_experiment_calibration_flag_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4", "--sparse", "4", "--sparse_steps", "3",
            "--hmc", "--hmc_chains", "2", "--hmc_tune", "6", "--hmc_draws", "5", "--holdout", "5"]
    eng = SgprQuantileDouble()
    s = mod.main(base + ["--calibration", "--out", str(tmp_path / "cal")], engine=eng)
    new = ["%s_%s_%s" % (c, m, k) for c in ("size", "noise") for m in ("ml2", "hmc", "sparse", "sparse_hmc") for k in ("cover95", "width95")]
    for k in new:
        assert len(s[k]) == 1 and np.isfinite(s[k]).all(), k
        assert (0.0 <= s[k][0] <= 1.0) if k.endswith("cover95") else s[k][0] > 0.0, (k, s[k])
    assert eng.calls["mixture_quantiles"] == 8 == eng.calls["exact_mixture"]   # per cell: four predictives, one call each
    z = np.load(tmp_path / "cal" / "hyperparameter_identification.npz")
    for c in ("size", "noise"):
        for m in ("learn", "hmc", "sparse", "sparse_hmc"):
            assert z["%s_%s_cover95" % (c, m)].shape == z["%s_%s_width95" % (c, m)].shape == (1, 2)
    # without the flag nothing changes: no new key, no new call, the same held-out figures
    eng0 = SgprQuantileDouble()
    s0 = mod.main(base + ["--out", str(tmp_path / "plain")], engine=eng0)
    assert eng0.calls["mixture_quantiles"] == 0 and set(s0) == set(s) - set(new)
    for k in s0:
        if k.endswith(("_nlpd", "_rmse")):
            assert s0[k] == s[k], k
    z0 = np.load(tmp_path / "plain" / "hyperparameter_identification.npz")
    assert set(z0.files) == {k for k in z.files if not k.endswith(("_cover95", "_width95"))}
    with pytest.raises(SystemExit):
        mod.main(base[:-2] + ["--calibration", "--out", str(tmp_path / "bad")], engine=SgprQuantileDouble())
