"""CPU: the batched collapsed bound around its kernel -- the ABI of libsgp_vfe_batch_hip.so, the host-side refusals, the float64 table
the GPU test (tests/test_vfe_batch_gpu.py) takes its tolerances from and deliberate defects failing that comparison, ``elbo_surface``
and ``fit_sgpr_batch`` on the CPU double (tests/vfe_batch_double.py), and the host-compilable part of csrc/sgp_vfe_batch.hpp as a
stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import vfe_batch_double as D
import vfe_reference as V
from conftest import ROOT
from vfe_batch_double import VfeBatchDouble

import ggp_amd
import ggp_amd._lib as L
from ggp_amd import sgpr_batch as SB

CSRC = os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc")
NAMES = {"sgp_vfe_batch_workspace_bytes": 6, "sgp_vfe_batch_occupancy": 2, "sgp_vfe_eval_batch": 25, "sgp_ctx_vfe_eval_batch": 26}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load_vfe_batch_library()


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_exported_and_bound(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgp_vfe_batch.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sgp_[a-z0-9_]+)\s*\(", txt))) == sorted(NAMES) == sorted(L.VFE_BATCH_PROTOTYPES)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.VFE_BATCH_PROTOTYPES[name][1]), name
        assert hasattr(lib, name), name
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", L.VFE_BATCH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(NAMES)
    und = subprocess.run([nm, "-D", "--undefined-only", L.VFE_BATCH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert [ln.split()[-1] for ln in und.splitlines() if re.search(r"\bsgp_", ln)] == ["sgp_ctx_device"]   # all it takes from the core
    core = open(os.path.join(ROOT, "include", "sgp.h")).read()
    assert not any(re.search(r"\b%s\b" % n, core) for n in NAMES) and L.SGP_ABI_VERSION == 3 and len(L.PROTOTYPES) == 146
    for table in (L.PROTOTYPES, L.EXACT_NUTS_PROTOTYPES, L.EXACT_PREDICT_PROTOTYPES):
        assert not any(n in table for n in NAMES)
    assert hasattr(ggp_amd.HipEngine, "vfe_eval_batch")
    import ggp_amd.build as B
    assert B.COMPANIONS == [("libsgp_exact_nuts_hip.so", ["sgp_exact_nuts.hip"], "sgp_exact_nuts.h"),
                            ("libsgp_exact_predict_hip.so", ["sgp_exact_predict.hip"], "sgp_exact_predict.h"),
                            ("libsgp_vfe_batch_hip.so", ["sgp_vfe_batch.hip"], "sgp_vfe_batch.h"),
                            ("libsgp_vfe_nuts_hip.so", ["sgp_vfe_nuts.hip"], "sgp_vfe_nuts.h"),
                            ("libsgp_vfe_predict_hip.so", ["sgp_vfe_predict.hip"], "sgp_vfe_predict.h")]
    assert "sgp_vfe_batch.hip" not in B.SOURCES


def test_the_digest_covers_the_new_library(lib, tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("_sgp_build_vb", os.path.join(ROOT, "generalised-gaussian-processes_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    (name, sources, header), = [c for c in b.COMPANIONS if c[0] == "libsgp_vfe_batch_hip.so"]
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
    for edited in (work / "sgp_vfe_batch.hip", work / "sgp_vfe_batch.hpp", work / "sgp_wg_dense.hpp", work / "sgp_common.hpp",
                   tmp_path / "include" / header):
        with open(edited, "a") as fh:
            fh.write("// a comment\n")
        after = b._companion_digest(b._digest(), sources, header)
        assert after != before, edited
        before = after


# ---------------------------------------------------------------------------------------------------------------- refusals, no device
def _eval_args(**bad):
    a = dict(ptr=8, P=2, N=10, M=5, d=2, kid=0, ws=8, nbytes=256, ldx=2, ldz=2, jitter=1e-6, out=8)
    a.update(bad)
    p = C.c_void_p(a["ptr"])  # (the dummy 8 is never dereferenced: every call here fails validation first)
    return (p, 20, a["ldx"], p, 10, None, None, p, 10, a["ldz"], None, p, a["P"], a["N"], a["M"], a["d"], a["kid"], a["jitter"], 1,
            C.c_void_p(a["out"]), None, p, C.c_void_p(a["ws"]), a["nbytes"], None)


def test_out_of_range_arguments_are_refused_on_the_host(lib):
    q = lib.sgp_vfe_batch_workspace_bytes
    assert q(2, 10, 5, 2, 1, 1) == 256 and q(2 ** 24 - 1, 65536, 64, 8, 1, 1) == 256 and q(1, 1, 1, 1, 0, 0) == 256
    assert q(2, 10, 3, 2, 1, 0) == 256   # M > N is legal
    for bad in ((0, 10, 5, 2), (2 ** 24, 10, 5, 2), (2, 0, 5, 2), (2, 65537, 5, 2), (2, 10, 0, 2), (2, 10, 65, 2), (2, 10, 5, 0), (2, 10, 5, 9)):
        assert q(*bad, 1, 1) == 0, bad
    for bad, status in ((dict(M=65), -2), (dict(M=0), -1), (dict(N=65537), -2), (dict(N=0), -1), (dict(d=9, ldx=9, ldz=9), -2), (dict(d=0), -1),
                        (dict(P=2 ** 24), -2), (dict(P=0), -1), (dict(kid=3), -1), (dict(kid=-1), -1), (dict(ptr=0), -1), (dict(out=0), -1),
                        (dict(ldx=1), -1), (dict(ldz=1), -1), (dict(jitter=-1e-6), -1), (dict(jitter=float("nan")), -1),
                        (dict(nbytes=255), -3), (dict(ws=0), -3),
                        # the order: SGP_ERR_ARG before SGP_ERR_DIM before SGP_ERR_WORKSPACE
                        (dict(M=65, ptr=0), -1), (dict(M=65, kid=3), -1), (dict(N=65537, ldx=1), -1), (dict(M=65, ws=0), -2),
                        (dict(P=2 ** 24, nbytes=0), -2), (dict(kid=3, ws=0), -1)):
        assert lib.sgp_vfe_eval_batch(*_eval_args(**bad)) == status, bad
        assert lib.sgp_ctx_vfe_eval_batch(None, *_eval_args(**bad)) == status, bad
    occ = lib.sgp_vfe_batch_occupancy
    assert occ(65, 0) == -2 and occ(0, 0) == -1 and occ(10, 3) == -1 and occ(10, -1) == -1 and occ(65, 3) == -1


def test_host_side_errors_carry_the_limits():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((20, 2)), rng.standard_normal(20)
    eng = VfeBatchDouble()
    with pytest.raises(ValueError, match="M <= 64"):
        ggp_amd.elbo_surface(X, y, rng.standard_normal((65, 2)), 1.0, 1.0, 0.1, engine=eng)
    with pytest.raises(ValueError, match="d <= 8"):
        ggp_amd.elbo_surface(rng.standard_normal((20, 9)), y, rng.standard_normal((5, 9)), 1.0, 1.0, 0.1, engine=eng)
    with pytest.raises(ValueError, match="N <= 65536"):
        ggp_amd.fit_sgpr_batch(np.zeros((65537, 1)), np.zeros(65537), np.zeros((3, 1)), max_steps=1, engine=eng)
    with pytest.raises(ValueError, match="20 rows"):
        ggp_amd.elbo_surface(X, y[:19], X[:5], 1.0, 1.0, 0.1, engine=eng)
    with pytest.raises(ValueError, match="rbf, matern32, matern52"):
        ggp_amd.elbo_surface(X, y, X[:5], 1.0, 1.0, 0.1, kernel="composite", engine=eng)
    with pytest.raises(ValueError, match="M <= N"):
        ggp_amd.fit_sgpr_batch(X[:4], y[:4], rng.standard_normal((5, 2)), n_restarts=1, max_steps=1, engine=eng)
    assert eng.calls["vfe_eval_batch"] == 0


# ---------------------------------------------------------------------------------------------------------------- the tolerance table
@pytest.mark.parametrize("name", D.CELLS)
def test_measured_e64_matches_the_table(name):
    """``measure_e64`` recomputes the float64 level of every cell and output group: the table of tests/test_vfe_batch_gpu.py holds it to
    one significant digit (the rule of tests/test_vfe_reference.py; below 1e-16 the figure is the rounding of single operations and
    need not reproduce).  The reference is finite at every cell."""
    import test_vfe_batch_gpu as G
    ref, A = D.reference(name)
    assert all(np.isfinite(np.asarray(ref[k], np.float64)).all() and np.isfinite(np.asarray(A[k], np.float64)).all() for k in D.GROUPS)
    e = D.measure_e64(name)
    assert set(G.E64) == set(D.CELLS) and set(G.E64[name]) == set(D.GROUPS)
    for k, want in G.E64[name].items():
        assert 0.4 * want <= e[k] <= 1.6 * want or max(e[k], want) < 1e-16, (name, k, e[k], want)


def test_the_cells_are_the_issue_s_and_the_new_ones_follow_the_rule():
    assert all(n in V.CELLS for n in D.FROM_V) and len(D.CELLS) == 23 and not any(n in V.CELLS for n in D.NEW)
    for n, c in D.NEW.items():
        assert (c["sf2"], c["s2"], c["jitter"], c["seed"]) == (1.3, 0.07, 1e-6, 1000 * c["N"] + 10 * c["M"] + c["d"]) and c["M"] <= 64
        inp = D.inputs(n)
        assert inp["X"].shape == (c["N"], c["d"]) and inp["Z"].shape == (c["M"], c["d"]) and inp["theta"].shape == (c["d"] + 2,)
    assert D.NEW["17-31-2-rbf"]["ls"] == [0.4, 0.44] and D.NEW["100-64-1-rbf"]["ls"] == [0.05]
    # the rule reproduces vfe_reference's own inputs where both can be asked
    c = V.CELLS["65-17-2-rbf"]
    rs = np.random.RandomState(c["seed"])
    X = rs.standard_normal((65, 2))
    assert np.array_equal(X, V.cell_inputs("65-17-2-rbf")["X"])


def test_the_hetero_problems_lie_below_the_floor():
    """The five problems of the GPU test's heterogeneous batch that are held to the reference: their float64 level is below FLOOR, so
    the tolerance there is MARGIN * FLOOR."""
    import test_vfe_batch_gpu as G
    X, Y, Z, theta, ix, iy, iz = G.hetero_problem()
    d = 2
    for p in (0, 7, 19, 30, 36):
        a = (X[ix[p]], Y[iy[p]], Z[iz[p]], theta[p, :d], theta[p, d], theta[p, d + 1], 1e-6, "matern52")
        ref, A = V.stationary(*a)
        for order in ("inverse", "substitution"):
            w = V.worst(V.stationary(*a, np.float64, order)[0], ref, A, D.GROUPS)
            assert max(w.values()) < V.FLOOR, (p, order, w)


@pytest.mark.parametrize("mutate", ["drop_row", "no_gg_kuu", "kuu_z_once", "no_jitter"])
def test_a_mutated_reference_stands_above_the_tolerance(mutate):
    """One deliberate defect at a time, at well-conditioned cells of the three size classes: the comparison of the GPU test fails on it."""
    import test_vfe_batch_gpu as G
    for name in ("65-17-2-rbf", "63-15-2-rbf", "200-64-2-matern32", "33-32-8-matern52"):
        ref, A = D.reference(name)
        bad, _ = D.evaluate(name, mutate=mutate)
        w = V.worst(bad, ref, A, D.GROUPS)
        over = {k: w[k] / V.tolerance(G.E64[name][k]) for k in w}
        print("MUTATION %s at %s: worst / tol = %.3g at %s" % (mutate, name, max(over.values()), max(over, key=over.get)))
        assert max(over.values()) > 1.0, (mutate, name, over)
        with pytest.raises(AssertionError):
            G.check(name, bad, ref, A, G.E64[name])


def test_the_double_meets_the_tolerance_and_reports_failures():
    import test_vfe_batch_gpu as G
    eng = VfeBatchDouble()
    for name in ("65-17-2-rbf", "33-32-8-matern52", "16-1-1-matern52"):
        inp = D.inputs(name)
        out, gz, info = eng.vfe_eval_batch(inp["X"], inp["y"], inp["Z"], inp["theta"][None], kernel=inp["kernel"], jitter=inp["jitter"],
                                           want_gz=True)
        assert int(info[0]) == 0
        G.check(name, D.unpack(out[0].numpy(), gz[0].numpy(), inp["X"].shape[1]), *D.reference(name), G.E64[name])
        out0, gz0, _ = eng.vfe_eval_batch(inp["X"], inp["y"], inp["Z"], inp["theta"][None], kernel=inp["kernel"], jitter=inp["jitter"],
                                          want_grad=False, want_gz=True)
        d = inp["X"].shape[1]
        assert gz0 is None and bool(out0[0, 1:d + 3].isnan().all()) and torch.equal(out0[0, [0, d + 3, d + 4]], out[0, [0, d + 3, d + 4]])
    inp = D.inputs("65-17-2-rbf")
    th = np.tile(inp["theta"], (5, 1))
    th[1, 0], th[2, 2], th[3, 3], th[4, 1] = np.nan, 0.0, -1.0, np.inf
    out, _, info = eng.vfe_eval_batch(inp["X"], inp["y"], inp["Z"], th)
    assert info.tolist() == [0, 1, 1, 1, 1] and bool(out[1:].isnan().all()) and bool(out[0].isfinite().all())
    with pytest.raises(ValueError):
        eng.vfe_eval_batch(inp["X"], inp["y"], inp["Z"], th, iz=[1] * 5)


# ---------------------------------------------------------------------------------------------------------------- elbo_surface
def test_elbo_surface_broadcasting_ard_empty_and_nan_cells():
    inp = D.inputs("65-17-2-rbf")
    X, y, Z = inp["X"], inp["y"], inp["Z"]
    eng = VfeBatchDouble()
    sf2, ls, s2 = np.array([0.5, 1.0, 2.0, 3.0])[:, None], np.array([0.7, 0.9, 1.1])[None, :], 0.07   # (a trailing axis of d = 2 would be ARD)
    F = ggp_amd.elbo_surface(X, y, Z, sf2, ls, s2, engine=eng)
    assert F.shape == (4, 3) and eng.calls["vfe_eval_batch"] == 1   # one launch
    Fp, lm, tr = ggp_amd.elbo_surface(X, y, Z, sf2, ls, s2, parts=True, engine=eng)
    assert np.array_equal(Fp, F) and np.allclose(lm - tr, F, rtol=1e-14)
    for i in range(4):   # cell by cell against the double
        for j in range(3):
            row, _ = D.one_row(X, y, Z, np.array([ls[0, j], ls[0, j], sf2[i, 0], s2]), 1e-6, "rbf", want_grad=False)
            assert (F[i, j], lm[i, j], tr[i, j]) == (row[0], row[5], row[6])
    # ARD: a trailing axis of length d that takes no part in the broadcast
    ard = np.array([[0.7, 1.3], [1.1, 0.9]])
    Fa = ggp_amd.elbo_surface(X, y, Z, sf2, ard[None], s2, kernel="matern32", engine=eng)
    assert Fa.shape == (4, 2)
    row, _ = D.one_row(X, y, Z, np.array([1.1, 0.9, 2.0, s2]), 1e-6, "matern32", want_grad=False)
    assert Fa[2, 1] == row[0]
    assert ggp_amd.elbo_surface(X, y, Z, 1.0, 1.0, 0.1, engine=eng).shape == ()
    # the empty grid: no launch
    n = eng.calls["vfe_eval_batch"]
    E = ggp_amd.elbo_surface(X, y, Z, np.zeros((0, 1)), ls, s2, engine=eng)
    Ep = ggp_amd.elbo_surface(X, y, Z, np.zeros((0, 1)), ls, s2, parts=True, engine=eng)
    assert E.shape == (0, 3) and len(Ep) == 3 and Ep[2].shape == (0, 3) and eng.calls["vfe_eval_batch"] == n
    # NaN cells: a non-positive hyper-parameter is reported by the kernel, not raised
    Fn = ggp_amd.elbo_surface(X, y, Z, np.array([1.0, -1.0, 0.0]), 1.0, 0.07, engine=eng)
    assert np.isfinite(Fn[0]) and np.isnan(Fn[1:]).all()
    with pytest.raises(ValueError, match="do not broadcast"):
        ggp_amd.elbo_surface(X, y, Z, np.ones(3), np.ones(4), 0.1, engine=eng)
    # d = 1 given as vectors
    inp1 = D.inputs("130-49-1-rbf")
    F1 = ggp_amd.elbo_surface(inp1["X"][:, 0], inp1["y"], inp1["Z"][:, 0], 1.3, np.array([0.05, 0.1]), 0.07, engine=eng)
    assert F1.shape == (2,) and abs(F1[0] - float(D.reference("130-49-1-rbf")[0]["F"])) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- fit_sgpr_batch
def test_one_adam_step_equals_torch_optim_adam():
    """Fed the same gradients, ``adam_step`` follows torch.optim.Adam to 1e-15 relative, step after step."""
    g = torch.Generator().manual_seed(0)
    P, K, steps, lr = 5, 7, 12, 0.01
    par = torch.randn(P, K, dtype=torch.float64, generator=g)
    ref = torch.nn.Parameter(par.clone())
    opt = torch.optim.Adam([ref], lr=lr)
    m, v, t = torch.zeros_like(par), torch.zeros_like(par), torch.zeros(P, dtype=torch.int64)
    pow1 = torch.tensor([0.9 ** k for k in range(steps + 1)], dtype=torch.float64)
    pow2 = torch.tensor([0.999 ** k for k in range(steps + 1)], dtype=torch.float64)
    ok = torch.ones(P, dtype=torch.bool)
    for _ in range(steps):
        grad = torch.randn(P, K, dtype=torch.float64, generator=g) * 10.0 ** torch.randint(-6, 3, (P, 1), generator=g).double()
        ref.grad = grad.clone()
        opt.step()
        SB.adam_step(par, grad, m, v, t, ok, lr, pow1, pow2)
        assert float(((par - ref.detach()).abs() / ref.detach().abs()).max()) <= 1e-15
    assert t.tolist() == [steps] * P


def _toy(B=3, N=40, M=6, d=2, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, N, d))
    Y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, N))
    return X, Y, X[:, :M].copy()


def test_fit_in_a_batch_is_the_fit_alone_and_seeds_reproduce():
    X, Y, Z = _toy()
    eng = VfeBatchDouble()
    fit = ggp_amd.fit_sgpr_batch(X, Y, Z, n_restarts=2, max_steps=6, lr=0.05, seed=7, engine=eng)
    assert eng.calls["vfe_eval_batch"] == fit.n_launches == 7   # one launch per step, one for the final bounds
    assert fit.losses.shape == (6, 3, 3) and fit.theta_all.shape == (3, 3, 4) and fit.Z_all.shape == (3, 3, 6, 2) and fit.elbo_all.shape == (3, 3)
    assert fit.theta.shape == (3, 4) and fit.Z.shape == (3, 6, 2) and fit.n_bad_steps.tolist() == [[0] * 3] * 3 and fit.seed == 7
    alone = ggp_amd.fit_sgpr_batch(X[0], Y[0], Z[0], n_restarts=2, max_steps=6, lr=0.05, seed=7, engine=VfeBatchDouble())
    for a, b in ((alone.losses[:, 0], fit.losses[:, 0]), (alone.theta_all[0], fit.theta_all[0]), (alone.Z_all[0], fit.Z_all[0]),
                 (alone.elbo_all[0], fit.elbo_all[0])):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))   # bit for bit
    one = ggp_amd.fit_sgpr_batch(X[1], Y[1], Z[1], max_steps=6, lr=0.05, seed=99, engine=VfeBatchDouble())   # start 0 draws nothing
    assert np.array_equal(one.losses[:, 0, 0].view(np.int64), fit.losses[:, 1, 0].view(np.int64))
    # elbo is the arg-max over the starts, and the best start's parameters are reported
    assert np.array_equal(fit.elbo, fit.elbo_all.max(1)) and np.array_equal(fit.best, fit.elbo_all.argmax(1))
    for b in range(3):
        assert np.array_equal(fit.theta[b], fit.theta_all[b, fit.best[b]]) and np.array_equal(fit.Z[b], fit.Z_all[b, fit.best[b]])
    assert (fit.elbo_all > -40 * fit.losses[0]).all()   # six steps of Adam went uphill
    # the starts: 0 is (raw = 0, Z_init); r >= 1 draws raw ~ N(0, 1) and M distinct rows of its data set from (seed, b, r)
    raw, Z1 = SB.sgpr_start(X[2], Z[2], 7, 2, 1)
    rng = np.random.default_rng([7, 2, 1])
    assert np.array_equal(raw, rng.standard_normal(4)) and np.array_equal(Z1, X[2][rng.choice(40, 6, replace=False)])
    assert len({tuple(r) for r in Z1}) == 6 and all(any(np.array_equal(r, x) for x in X[2]) for r in Z1)
    raw0, Z0 = SB.sgpr_start(X[2], Z[2], 7, 2, 0)
    assert not raw0.any() and np.array_equal(Z0, Z[2])
    again = ggp_amd.fit_sgpr_batch(X, Y, Z, n_restarts=2, max_steps=6, lr=0.05, seed=7, engine=VfeBatchDouble())
    other = ggp_amd.fit_sgpr_batch(X, Y, Z, n_restarts=2, max_steps=6, lr=0.05, seed=8, engine=VfeBatchDouble())
    assert np.array_equal(again.losses, fit.losses) and np.array_equal(again.Z_all, fit.Z_all)
    assert np.array_equal(other.losses[:, :, 0], fit.losses[:, :, 0]) and not np.array_equal(other.losses[:, :, 1:], fit.losses[:, :, 1:])


def test_the_parametrisation_and_the_loss_are_train_model_s():
    """Step 0 evaluates theta = [softplus(0)] * (d + 1) + [softplus(0) + 1e-4] at Z_init, the loss is -F / N, and the first update is
    torch.optim.Adam's on the raw parameters and Z with the chain rule through softplus."""
    X, Y, Z = _toy(B=1)
    sp = float(np.log(2.0))
    fit0 = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=0, engine=VfeBatchDouble())
    assert np.array_equal(fit0.theta[0], np.array([sp, sp, sp, sp + 1e-4])) and np.array_equal(fit0.Z[0], Z[0]) and fit0.losses.shape == (0, 1, 1)
    row, gz = D.one_row(X[0], Y[0], Z[0], fit0.theta[0], 1e-6, "rbf")
    assert fit0.elbo[0] == row[0]
    fit1 = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=1, lr=0.01, engine=VfeBatchDouble())
    assert fit1.losses[0, 0, 0] == -row[0] / 40
    raw = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    Zp = torch.nn.Parameter(torch.as_tensor(Z[0]).clone())
    opt = torch.optim.Adam([raw, Zp], lr=0.01)
    raw.grad = torch.as_tensor(-row[1:5] / 40) * torch.sigmoid(raw.detach())
    Zp.grad = torch.as_tensor(-gz / 40)
    opt.step()
    th = torch.nn.functional.softplus(raw.detach()).numpy() + np.array([0, 0, 0, 1e-4])
    assert np.allclose(fit1.theta[0], th, rtol=1e-15, atol=0) and np.allclose(fit1.Z[0], Zp.detach().numpy(), rtol=1e-14, atol=1e-16)
    fixed = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=3, learn_Z=False, engine=VfeBatchDouble())
    assert np.array_equal(fixed.Z[0], Z[0]) and not np.array_equal(fixed.theta[0], fit0.theta[0])


def test_a_failed_problem_keeps_its_parameters_for_that_step():
    X, Y, Z = _toy()
    kw = dict(n_restarts=1, lr=0.05, seed=1)
    bad = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=5, engine=VfeBatchDouble(fail=lambda call, p: call == 2 and p == 3), **kw)
    good = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=4, engine=VfeBatchDouble(), **kw)
    assert bad.n_bad_steps.reshape(-1).tolist() == [0, 0, 0, 1, 0, 0] and np.isnan(bad.losses[2, 1, 1]) and np.isfinite(bad.losses).sum() == 29
    # the skipped step changed nothing: problem 3 after 5 steps with one skipped is problem 3 after 4 steps
    assert np.array_equal(bad.theta_all[1, 1], good.theta_all[1, 1]) and np.array_equal(bad.Z_all[1, 1], good.Z_all[1, 1])
    assert np.array_equal(bad.losses[[0, 1, 3, 4], 1, 1], good.losses[:, 1, 1])
    # ... and its neighbours took all five
    five = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=5, engine=VfeBatchDouble(), **kw)
    keep = np.ones((3, 2), bool)
    keep[1, 1] = False
    assert np.array_equal(bad.theta_all[keep], five.theta_all[keep]) and not np.array_equal(bad.theta_all[1, 1], five.theta_all[1, 1])
    # a start whose final evaluation fails never wins
    last = ggp_amd.fit_sgpr_batch(X, Y, Z, max_steps=2, engine=VfeBatchDouble(fail=lambda call, p: call == 2 and p == 0), **kw)
    assert np.isnan(last.elbo_all[0, 0]) and last.best[0] == 1 and last.elbo[0] == last.elbo_all[0, 1]


def test_model_carries_the_parameters():
    X, Y, Z = _toy(d=2)
    for kernel in ("rbf", "matern32"):
        fit = ggp_amd.fit_sgpr_batch(X, Y, Z, kernel=kernel, max_steps=3, lr=0.05, seed=0, engine=VfeBatchDouble())
        m = fit.model(2)
        assert isinstance(m, ggp_amd.SparseGPR) and m.base_covar_module.base_kernel.kernel_name == kernel and m.jitter == 1e-6
        ls, sf2, s2 = m._hypers()
        assert np.allclose(ls + [sf2, s2], fit.theta[2], rtol=1e-12, atol=0)
        assert np.array_equal(m.inducing_points.numpy(), fit.Z[2]) and np.array_equal(m.train_x.numpy(), X[2])
        assert np.array_equal(m.train_y.numpy(), Y[2])
    bare = ggp_amd.SgprBatchResult(**{**fit.__dict__, "X": None})
    with pytest.raises(ValueError, match="does not carry the data"):
        bare.model(0)


def test_experiment_sparse_flag_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from exact_predict_double import ExactPredictDouble

    class Both(ExactPredictDouble, VfeBatchDouble):
        def __init__(self):
            ExactPredictDouble.__init__(self)
            self.fail = None
            self.calls["vfe_eval_batch"] = 0

    base = ["--sizes", "10", "--noise_vars", "1", "--n_sets", "2", "--grid", "4"]
    eng = Both()
    s = mod.main(base + ["--sparse", "4", "--sparse_steps", "5", "--out", str(tmp_path / "sparse")], engine=eng)
    z = np.load(tmp_path / "sparse" / "hyperparameter_identification.npz")
    for c in ("size", "noise"):
        for k in ("ls", "sf", "sn", "elbo"):
            assert z["%s_sparse_%s" % (c, k)].shape == (1, 2) and np.isfinite(z["%s_sparse_%s" % (c, k)]).all()
    assert eng.calls["vfe_eval_batch"] == 2 * 6   # per cell: five steps and the final bounds, all data sets in each launch
    eng0 = Both()
    s0 = mod.main(base + ["--out", str(tmp_path / "plain")], engine=eng0)
    z0 = np.load(tmp_path / "plain" / "hyperparameter_identification.npz")
    assert eng0.calls["vfe_eval_batch"] == 0 and not any("sparse" in k for k in z0.files) and set(s0) <= set(s)
    assert np.array_equal(z0["size_learn_ls"], z["size_learn_ls"])


# ---------------------------------------------------------------------------------------------------------------- the host program
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]


def test_host_part_of_the_header_under_asan_ubsan(tmp_path):
    """tests/native/vfe_batch_host.cpp (its own main) over the plain-C++ part of csrc/sgp_vfe_batch.hpp: size class, tile geometry,
    workspace query, refusals, theta-row validation.  Built by g++ alone and run directly."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("sanitizer builds run on CPU-only hosts, never on a GPU box")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "vfe_batch_host_asan")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-I", CSRC, "-o", exe,
                                                                           os.path.join(ROOT, "tests", "native", "vfe_batch_host.cpp")],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "vfe batch host ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
