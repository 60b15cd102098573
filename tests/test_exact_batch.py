"""CPU: the batched exact-GP marginal likelihood above the engine seam -- the yardsticks themselves (the float64 double against the
long-double reference), ``lml_surface`` and ``fit_ml2`` against the scikit-learn fixtures of tests/golden/make_golden_ml2_sklearn.py, the
argument handling, the experiment driver at a toy size and the binding of the new symbols."""
import importlib.util
import itertools
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from exact_batch_double import ExactBatchDouble
from exact_batch_reference import TAU, ratios, reference

import ggp_amd
from ggp_amd import _lib as L

SK = os.path.join(GOLDEN_DIR, "sklearn")


def load(name):
    z = np.load(os.path.join(SK, name + ".npz"))
    return {k: z[k] for k in z.files}


def ml2_cells():
    z = load("ml2_fits")
    return [{k[len("c%d_" % c):]: v for k, v in z.items() if k.startswith("c%d_" % c)} for c in range(int(z["n_cells"]))]


def surface_theta(G, name):
    sf2, ls = G[name + "_sf2"], G[name + "_ls"]
    return sf2, ls, float(G[name + "_s2"])


def check_surface(got, G, name):
    """|lml_surface - scikit-learn| <= TAU S_F at every cell (S_F from the long-double reference at that cell)."""
    sf2, ls, s2 = surface_theta(G, name)
    assert got.shape == G[name + "_lml"].shape and not np.isnan(got).any()
    worst = 0.0
    for i, j in itertools.product(range(sf2.size), range(ls.size)):
        ref = reference(G[name + "_X"], G[name + "_y"], [ls[j]], sf2[i], s2)
        worst = max(worst, abs(got[i, j] - G[name + "_lml"][i, j]) / float(ref["S_F"]))
    assert worst <= TAU, "%s: worst |lml - sklearn| / S_F = %.3e" % (name, worst)


def check_ml2(res, cell):
    """The three conditions on a fit from the fixture's starts: best-of-starts no worse than scikit-learn's, at least 9 of 11 starts
    converged, and the projected gradient -- from the long-double reference, not from the code under test -- small at each of them."""
    X, Y, bounds, sk = cell["X"], cell["Y"], cell["bounds"], cell["sk_lml"]
    N, d = X.shape
    free = np.ones(d + 2, dtype=bool)
    free[-1] = str(cell["noise"]) == "learn"
    lo, hi = np.log(bounds[:, 0]), np.log(bounds[:, 1])
    for b in range(Y.shape[0]):
        assert res.lml[b] >= sk[b] - 1e-6 * (abs(sk[b]) + N), "set %d: %.12g below scikit-learn's %.12g" % (b, res.lml[b], sk[b])
        assert res.converged[b].sum() >= 9, "set %d: %d of %d starts converged" % (b, res.converged[b].sum(), res.converged.shape[1])
        for s in np.nonzero(res.converged[b])[0]:
            th = res.theta_all[b, s]
            ref = reference(X, Y[b], th[:d], th[d], th[d + 1])
            z = np.log(th)
            g = -(np.asarray(ref["g"], dtype=np.float64) * th)
            pg = np.abs((z - np.clip(z - g, lo, hi))[free]).max()
            assert pg <= 1e-4, "set %d start %d: projected gradient %.3g" % (b, s, pg)


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def sweep_theta():
    return itertools.product([0.1, 25.0, 1e3, 1e5], [0.1, 2.0, 1e2, 1e5], [0.1, 1.0, 9.0])


@pytest.mark.parametrize("N,d,kernel", list(itertools.product([1, 5, 17, 30, 65, 120, 128], [1, 2, 8], ["rbf", "matern52"])))
def test_the_float64_double_is_within_a_hundredth_of_tau_of_long_double(N, d, kernel):
    """The textbook float64 evaluation over the whole sweep -- every N x d x kernel cell, and in each all 4 sf2 x 4 ls x 3 s2 = 48 rows
    of theta, the corners of the reference's grids (cond up to 1.2e8) among them; nothing is thinned.  The yardstick of the CPU suite is
    itself held to TAU / 100 in the measure every other test uses (the worst of the method: about 3e-15 for F, 6e-15 for the gradient).

    The inputs are a walk whose steps cycle through 0.03, 0.095, 0.3, 0.95, 3 in a random direction, so that at every lengthscale of the
    sweep some pairs of points lie within a lengthscale of each other.  The measure models a relative perturbation of A's entries of the
    order of 2^-53; the float64 value of exp(-r^2 / 2) carries r^2 / 2 times that from the rounding of its argument alone.  Where every
    pair is ten and more lengthscales apart (points uniform in [0, 10]^d, d >= 2, at ls = 0.1) a lengthscale gradient is a sum of such
    terms only -- 1e-97 ... 1e-240 in size, 2e-14 ... 6e-14 off in this measure in ANY float64 code, within TAU but not TAU / 100."""
    rng = np.random.default_rng(N + d)
    dirs = rng.standard_normal((N, d))
    steps = 0.03 * 10.0 ** (0.5 * (np.arange(N) % 5))
    X = 5.0 + np.cumsum(steps[:, None] * dirs / np.linalg.norm(dirs, axis=1, keepdims=True), 0)
    y = 5.0 * rng.standard_normal(N)
    theta = np.array([[ls] * d + [sf2, s2] for sf2, ls, s2 in sweep_theta()])
    F, out, g, info = ExactBatchDouble().exact_eval_batch(X, y, theta, kernel=kernel)
    assert int(info.abs().sum()) == 0
    worst = [0.0, 0.0]
    for p in range(theta.shape[0]):
        rF, rg = ratios(float(F[p]), g[p].numpy(), reference(X, y, theta[p, :d], theta[p, d], theta[p, d + 1], kernel))
        worst = [max(worst[0], rF), max(worst[1], rg)]
    assert worst[0] <= TAU / 100 and worst[1] <= TAU / 100, worst


def test_reference_gradient_is_the_derivative_of_its_value():
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 10, (9, 2)), rng.standard_normal(9)
    th = np.array([1.3, 2.1, 4.0, 0.3])
    g = reference(X, y, th[:2], th[2], th[3], "matern32")["g"]
    for i in range(4):
        e = np.zeros(4)
        e[i] = 1e-6 * th[i]
        fd = (reference(X, y, (th + e)[:2], th[2] + e[2], th[3] + e[3], "matern32")["F"]
              - reference(X, y, (th - e)[:2], th[2] - e[2], th[3] - e[3], "matern32")["F"]) / (2 * e[i])
        assert abs(float(fd - g[i])) <= 1e-8 * max(1.0, abs(float(g[i])))


def test_double_reports_a_singular_problem_without_touching_its_neighbours():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((2, 12, 3))
    X[1, 6:] = X[1, :6]
    y = rng.standard_normal(12)
    theta = np.tile([1.0, 1.0, 1.0, 1.0, 0.1], (3, 1))
    theta[1, -1] = 1e-300
    F, out, g, info = ExactBatchDouble().exact_eval_batch(X, y, theta, ix=[0, 1, 0])
    assert info[1] != 0 and info[0] == 0 and info[2] == 0
    assert bool(F[1].isnan()) and bool(g[1].isnan().all()) and F[0] == F[2] and bool(g[0].isfinite().all())


def bad_theta_rows():
    """d = 2 rows [ls_1, ls_2 | sf2 | s2]: row 0 is healthy, every other has one entry that is not a positive finite number -- among them
    the ones a factorisation alone would let through (a negative lengthscale, sf2 = 0, a negative sf2 under a large s2)."""
    th = np.tile([1.5, 0.7, 2.0, 0.3], (8, 1))
    th[1, 0], th[2, 1], th[3, 2], th[4, 3] = -1.5, 0.0, 0.0, -0.3
    th[5, 2:] = -0.01, 5.0
    th[6, 3], th[7, 1] = np.nan, np.inf
    return th


def test_double_reports_a_theta_that_is_not_positive_and_finite():
    rng = np.random.default_rng(4)
    X, y = rng.uniform(0, 10, (6, 2)), rng.standard_normal(6)
    th = bad_theta_rows()
    F, out, g, info = ExactBatchDouble().exact_eval_batch(X, y, th)
    assert info.tolist() == [0] + [1] * 7 and bool(F[0].isfinite()) and bool(F[1:].isnan().all()) and bool(g[1:].isnan().all())
    got = ggp_amd.lml_surface(X, y, th[:, 2], th[:, :2], th[:, 3], engine=ExactBatchDouble())
    assert np.isfinite(got[0]) and np.isnan(got[1:]).all()


# ---------------------------------------------------------------------------------------------------------------- lml_surface
@pytest.mark.parametrize("name", ["a", "b"])
def test_lml_surface_matches_sklearn(name):
    G = load("lml_surface")
    sf2, ls, s2 = surface_theta(G, name)
    got = ggp_amd.lml_surface(G[name + "_X"], G[name + "_y"], sf2[:, None], ls[None, :], s2, engine=ExactBatchDouble())
    check_surface(got, G, name)


def test_lml_surface_broadcasting_and_errors():
    eng = ExactBatchDouble()
    rng = np.random.default_rng(0)
    X, y = rng.uniform(0, 10, (6, 2)), rng.standard_normal(6)
    a = ggp_amd.lml_surface(X, y, 2.0, 1.5, 0.3, engine=eng)
    assert a.shape == () and np.isfinite(a)
    ard = ggp_amd.lml_surface(X, y, np.array([2.0, 3.0])[:, None], np.array([[1.5, 1.5], [1.5, 0.7], [0.2, 0.7]]), 0.3, engine=eng)
    assert ard.shape == (2, 3) and ard[0, 0] == a and ard[0, 1] != a
    grid = ggp_amd.lml_surface(X, y, np.array([2.0, 3.0])[:, None, None], np.array([1.5, 0.7, 0.2])[None, :, None],
                               np.array([0.3, 1.0, 2.0, 3.0]), kernel="matern32", engine=eng)
    assert grid.shape == (2, 3, 4) and eng.calls["exact_eval_batch"] == 3
    one_d = ggp_amd.lml_surface(X[:, 0], y, [1.0, 2.0], 1.0, 0.1, engine=eng)
    assert one_d.shape == (2,)
    X2 = X.copy()
    X2[3:] = X2[:3]
    bad = ggp_amd.lml_surface(X2, y, 1.0, 1.0, [0.1, 1e-300], engine=eng)
    assert np.isfinite(bad[0]) and np.isnan(bad[1])
    with pytest.raises(ValueError):
        ggp_amd.lml_surface(X, y, np.ones(2), np.ones(3), 0.1, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.lml_surface(X, y[:5], 1.0, 1.0, 0.1, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.lml_surface(np.zeros((129, 1)), np.zeros(129), 1.0, 1.0, 0.1, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.lml_surface(np.zeros((4, 9)), np.zeros(4), 1.0, 1.0, 0.1, engine=eng)
    with pytest.raises(ValueError):
        ggp_amd.lml_surface(X, y, 1.0, 1.0, 0.1, kernel="composite", engine=eng)


# ---------------------------------------------------------------------------------------------------------------- fit_ml2
@pytest.fixture(scope="module")
def cells():
    return ml2_cells()


@pytest.mark.parametrize("c", range(5))
def test_fit_ml2_from_sklearns_starts_is_no_worse_than_sklearn(cells, c):
    cell = cells[c]
    eng = ExactBatchDouble()
    res = ggp_amd.fit_ml2(cell["X"], cell["Y"], noise=str(cell["noise"]), theta0=cell["theta0"], bounds=cell["bounds"],
                          starts=cell["starts"], engine=eng)
    assert eng.calls["exact_eval_batch"] == res.n_batches  # every trial step of every problem is one batched evaluation
    assert res.theta_all.shape == cell["starts"].shape[:1] + (11, cell["X"].shape[1] + 2) and (res.n_iter <= 200).all()
    if str(cell["noise"]) == "fixed":
        assert (res.theta_all[:, :, -1] == cell["theta0"][-1]).all()
    assert (res.theta_all >= cell["bounds"][:, 0] * (1 - 1e-12)).all() and (res.theta_all <= cell["bounds"][:, 1] * (1 + 1e-12)).all()
    check_ml2(res, cell)


def test_fit_ml2_draws_its_restarts_the_way_sklearn_does(cells):
    from sklearn.utils import check_random_state
    cell = cells[1]
    b = cell["bounds"]
    z = ggp_amd.ml2.draw_starts(np.log(b), np.ones(3, dtype=bool), 1, 10, int(cell["seeds"][0]))
    assert np.allclose(np.exp(z[0]), cell["starts"][0], rtol=1e-13)
    r = check_random_state(5)
    zf = ggp_amd.ml2.draw_starts(np.log(b), np.array([True, True, False]), 2, 3, 5)
    want = np.array([r.uniform(np.log(b[[1, 0], 0]), np.log(b[[1, 0], 1])) for _ in range(6)]).reshape(2, 3, 2)
    assert np.array_equal(zf[:, :, [1, 0]], want) and np.isnan(zf[:, :, 2]).all()
    X, Y = cell["X"], cell["Y"][:2]
    a = ggp_amd.fit_ml2(X, Y, theta0=cell["theta0"], bounds=b, n_restarts=3, seed=11, engine=ExactBatchDouble())
    a2 = ggp_amd.fit_ml2(X, Y, theta0=cell["theta0"], bounds=b, n_restarts=3, seed=11, engine=ExactBatchDouble())
    assert a.theta_all.shape == (2, 4, 3) and np.array_equal(a.theta_all, a2.theta_all) and (a.lml >= a.lml_all[:, 0]).all()
    assert (a.n_evals >= 4).all()


def test_fit_ml2_argument_errors(cells):
    cell = cells[0]
    X, Y, th0, b = cell["X"], cell["Y"][:2], cell["theta0"], cell["bounds"]
    eng = ExactBatchDouble()
    for kw in (dict(noise="estimate"), dict(kernel="composite"), dict(theta0=None), dict(bounds=None), dict(theta0=th0[:2]),
               dict(bounds=b[:, ::-1] * np.array([1.0, 2.0])), dict(starts=np.ones((3, 2))), dict(starts=-np.ones((3, 3))),
               dict(n_restarts=-1), dict(theta0=[1.0, -1.0, 1.0])):
        args = dict(theta0=th0, bounds=b, engine=eng)
        args.update(kw)
        with pytest.raises(ValueError):
            ggp_amd.fit_ml2(X, Y, **args)
    with pytest.raises(ValueError):
        ggp_amd.fit_ml2(X[:5], Y, theta0=th0, bounds=b, engine=eng)
    assert eng.calls["exact_eval_batch"] == 0


# ---------------------------------------------------------------------------------------------------------------- the experiment
def test_experiment_driver_at_a_toy_size(tmp_path):
    spec = importlib.util.spec_from_file_location("hyperparameter_identification",
                                                  os.path.join(ROOT, "experiments", "hyperparameter_identification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = mod.main(["--sizes", "10", "20", "--noise_vars", "1", "9", "--n_sets", "3", "--grid", "6", "--out", str(tmp_path)],
                 engine=ExactBatchDouble())
    z = np.load(tmp_path / "hyperparameter_identification.npz")
    assert z["size_learn_ls"].shape == (2, 3) and z["noise_fixed_sf"].shape == (2, 3) and z["surface_n10"].shape == (6, 6)
    assert (z["size_fixed_sn"] == 1.0).all() and np.allclose(z["noise_fixed_sn"][1], 3.0)
    assert np.isfinite(z["surface_n5"]).all() and np.isfinite(z["surface_noise"]).all() and s["surface_nan_cells"] == 0
    assert json.load(open(tmp_path / "hyperparameter_identification.json"))["sizes"] == [10, 20]


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_new_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp.h")).read()
    for name, nargs in (("sgp_exact_batch_workspace_bytes", 4), ("sgp_exact_batch_occupancy", 2), ("sgp_exact_eval_batch", 19),
                        ("sgp_ctx_exact_eval_batch", 20)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.PROTOTYPES[name][1]), name
    assert hasattr(ggp_amd.HipEngine, "exact_eval_batch") and L.SGP_ABI_VERSION == 3


def test_host_side_limits_of_the_batch_need_no_device():
    import __graft_entry__ as ge
    ge.build()
    lib = ggp_amd.load_library()
    q = lib.sgp_exact_batch_workspace_bytes
    assert q(1, 1, 1, 0) > 0 and q(2 ** 24 - 1, 128, 8, 1) > 0
    assert q(2 ** 24, 10, 2, 1) == 0 and q(0, 10, 2, 1) == 0 and q(4, 129, 1, 1) == 0 and q(4, 10, 9, 1) == 0
    null = None
    for P, N, d, kid, status in ((2 ** 24, 10, 2, 0, -2), (2, 129, 2, 0, -2), (2, 10, 9, 0, -2), (2, 10, 2, 3, -1), (0, 10, 2, 0, -1)):
        assert lib.sgp_exact_eval_batch(null, 0, d, null, 0, null, null, null, P, N, d, kid, 1, null, null, null, null, 0, null) == status
    assert lib.sgp_exact_batch_occupancy(129, 0) == -2 and lib.sgp_exact_batch_occupancy(10, 3) == -1


# ---------------------------------------------------------------------------------------------------------------- the shared intake
def test_the_batched_intake_lifts_checks_and_names_what_it_was_given():
    """``HipEngine._batch_intake`` and ``_set_index`` -- the intake of all six batched entry points -- on CPU tensors."""
    import torch
    cpu, f64 = torch.device("cpu"), torch.float64
    intake, set_index = ggp_amd.HipEngine._batch_intake, ggp_amd.HipEngine._set_index
    N, d, M, T, P = 6, 2, 3, 4, 5
    X, Y, Z, Xs, theta = (torch.zeros(s, dtype=f64) for s in ((N, d), (N,), (M, d), (T, d), (P, d + 2)))
    # one rank short is one set; a set-major tensor is taken as it is; None passes through
    tensors, idx, dims = intake(cpu, X, Y, Z, theta, Xs, (None, [0] * P, None, None))
    assert [tuple(t.shape) for t in tensors] == [(1, N, d), (1, N), (1, M, d), (1, T, d)]
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(tensors, (X, Y, Z, Xs)))
    assert idx[0] is idx[2] is idx[3] is None and idx[1].dtype == torch.int32 and idx[1].tolist() == [0] * P and dims == (N, d, M, T, P)
    X3, Y2, Z3, Xs3 = X.expand(2, N, d).contiguous(), Y.expand(3, N).contiguous(), Z.expand(4, M, d).contiguous(), Xs.expand(7, T, d).contiguous()
    top = ([1] * P, [2] * P, [3] * P, [6] * P)  # the last set of each of the 2, 3, 4 and 7
    tensors, idx, dims = intake(cpu, X3, Y2, Z3, theta, Xs3, top)
    assert all(a is b for a, b in zip(tensors, (X3, Y2, Z3, Xs3)))
    assert [i.tolist() for i in idx] == [list(i) for i in top] and dims == (N, d, M, T, P)
    for k, name in enumerate(("ix", "iy", "iz", "ixs")):  # each index against the set count of its own tensor
        with pytest.raises(ValueError, match=r"%s must hold 5 indices in \[0, %d\)" % (name, top[k][0] + 1)):
            intake(cpu, X3, Y2, Z3, theta, Xs3, top[:k] + ([top[k][0] + 1] * P,) + top[k + 1:])
    with pytest.raises(ValueError, match=r"ixs must hold 5 indices in \[0, 7\)"):  # without a Z the third index is the test set's
        intake(cpu, X3, Y2, theta=theta, Xs=Xs3, idx=(None, None, [7] * P))
    tensors, idx, dims = intake(cpu, X, Y2, theta=theta, idx=(None, None))
    assert tensors[1] is Y2 and tensors[2:] == (None, None) and idx == [None, None] and dims == (N, d, None, None, P)
    # the refusal names exactly the tensors passed, theta last
    for kw, text in (
            (dict(Y=torch.zeros(N + 1, dtype=f64), theta=theta), "shapes: X (1, 6, 2), Y (1, 7), theta (5, 4) (expected theta P x 4)"),
            (dict(Y=Y, Z=torch.zeros(M, d + 1, dtype=f64), theta=theta),
             "shapes: X (1, 6, 2), Y (1, 6), Z (1, 3, 3), theta (5, 4) (expected theta P x 4)"),
            (dict(Y=Y, theta=theta, Xs=torch.zeros(2, T, d - 1, dtype=f64)),
             "shapes: X (1, 6, 2), Y (1, 6), Xs (2, 4, 1), theta (5, 4) (expected theta P x 4)"),
            (dict(Y=Y, Z=Z, theta=torch.zeros(P, d + 1, dtype=f64), Xs=Xs),
             "shapes: X (1, 6, 2), Y (1, 6), Z (1, 3, 2), Xs (1, 4, 2), theta (5, 3) (expected theta P x 4)"),
            (dict(Y=Y, theta=torch.zeros(d + 2, dtype=f64)), "shapes: X (1, 6, 2), Y (1, 6), theta (4,) (expected theta P x 4)")):
        with pytest.raises(ValueError) as e:
            intake(cpu, X, **kw)
        assert str(e.value) == text
    # a sampler has no theta: its own arguments decide with the shapes and end the text; the VFE limits come after the shapes
    assert intake(cpu, X, Y, Z, own=(9, True, ""))[2] == (N, d, M, None, 9)
    for kw, fits, text in ((dict(Y=Y), False, "shapes: X (1, 6, 2), Y (1, 6), q0 (2, 4), 3 seeds, n_tune 0, n_draws 1"),
                           (dict(Y=Y[:-1], Z=Z), True, "shapes: X (1, 6, 2), Y (1, 5), Z (1, 3, 2), q0 (2, 4), 3 seeds, n_tune 0, n_draws 1")):
        with pytest.raises(ValueError) as e:
            intake(cpu, X, own=(2, fits, ", q0 (2, 4), 3 seeds, n_tune 0, n_draws 1"), **kw)
        assert str(e.value) == text
    with pytest.raises(ValueError, match=r"vfe_nuts_batch takes 1 <= M <= 64, .* and 1 <= C < 2\^24 \(got M 3, N 6, d 2, C 0\)"):
        intake(cpu, X, Y, Z, limits=("vfe_nuts_batch", "C"), own=(0, True, ""))
    with pytest.raises(ValueError, match=r"vfe_predict_batch takes .* 1 <= d <= 8, 1 <= T <= 32768 and 1 <= P < 2\^24 \(got M 65, N 6, d 2, T 4, P 5\)"):
        intake(cpu, X, Y, torch.zeros(65, d, dtype=f64), theta, Xs, limits=("vfe_predict_batch", "P"))
    for bad in (X.float(), X.t()):
        with pytest.raises(ValueError, match="X must be a contiguous float64 tensor on cpu"):
            intake(cpu, bad, Y, theta=theta)
    # the set indices: None passes through, a host sequence is range-checked, a tensor on the device is taken as it is
    assert set_index(cpu, None, "ix", 3, P) is None
    got = set_index(cpu, [0, 2, 1, 2, 0], "iy", 3, P)
    assert got.dtype == torch.int32 and got.tolist() == [0, 2, 1, 2, 0]
    own = torch.zeros(P, dtype=torch.int32)
    assert set_index(cpu, own, "iz", 3, P) is own
    for idx, text in (([0, 1], "ix must hold 5 indices in [0, 3)"), ([0, 1, 2, 3, 0], "ix must hold 5 indices in [0, 3)"),
                      (np.array([0, -1, 0, 0, 0]), "ix must hold 5 indices in [0, 3)"),
                      (torch.zeros(P, dtype=torch.int64), "ix must be a contiguous int32 tensor of 5 entries"),
                      (torch.zeros(P + 1, dtype=torch.int32), "ix must be a contiguous int32 tensor of 5 entries")):
        with pytest.raises(ValueError) as e:
            set_index(cpu, idx, "ix", 3, P)
        assert str(e.value) == text
