#!/usr/bin/env python3
"""The reference's hyper-parameter identification study (experiments/hyperparameter_identification.py and experiments/lml_surface.py)
on the batched exact-GP entry point: where ML-II fails, and why one samples theta instead.

  * data: draws of a GP prior (sig_f = 5, lengthscale 2) on a 500-point grid of [0, 10], observed with noise at n grid points chosen
    uniformly (or, ``--bimodal``, around 2 and 8) -- ``ggp_amd.identification_data``;
  * size sweep: ML-II (``ggp_amd.fit_ml2``: theta0 = 1, 10 restarts, lengthscale in [1e-2, 1e3]) on ``--n_sets`` data sets at each of
    ``--sizes`` training sizes, noise fixed at its true value and learnt;
  * noise sweep: the same at n = 30 for noise variances 1, 3, 6, 9 (5 restarts, lengthscale in [1e-2, 1e4]), fixed and learnt;
  * three LML surfaces (``ggp_amd.lml_surface``): (sf2, ls) at n = 5 and n = 10 with the noise at 1, and (ls, s2) at n = 30 with sf2 at
    its fitted value -- one launch each.

  * ``--hmc`` (off by default): the Bayesian answer beside every ML-II one -- NUTS over (log ls, log sig_f, log sig_n) on each data set
    of each cell (``ggp_amd.sample_exact_nuts_batch``: ``--hmc_chains`` chains of ``--hmc_tune`` + ``--hmc_draws`` draws per data set, all
    chains of a cell in one device-resident batch), recorded as the posterior means per data set;
  * ``--holdout K`` (0 by default): K more points per data set, kept out of the fit and the sampling: the held-out NLPD and RMSE of the
    ML-II plug-in (``Ml2Result.predict``) and, with ``--hmc``, of the mixture over the draws (``ExactNutsResult.predict``) -- whether
    sampling theta predicts better than plugging in its ML-II value (summary keys ``<sweep>_ml2_nlpd``, ``_hmc_nlpd``, ``_ml2_rmse``,
    ``_hmc_rmse``, one entry per cell);
  * ``--sparse M`` (0 by default): the sparse ML-II estimates beside the exact ones -- the collapsed bound with M inducing inputs
    (``ggp_amd.fit_sgpr_batch``, ``learn_Z=True``: Adam for ``--sparse_steps`` steps, all data sets of a cell in lock step with one
    launch per step), started at M evenly spaced training inputs; recorded as ``<sweep>_sparse_ls``, ``_sf``, ``_sn``, ``_elbo``;
  * ``--sparse M`` together with ``--hmc``: also NUTS over theta of the collapsed bound of every data set at its fitted Z
    (``SgprBatchResult.sample_nuts``: the reference's ``train_fixed_model`` protocol, all chains of a cell in one device-resident batch),
    the posterior means of (ls, sig_f, sig_n) recorded beside the sparse ML-II estimates as ``<sweep>_sparse_hmc_ls``, ``_sf``, ``_sn``
    and ``_seconds``;
  * ``--sparse M`` together with ``--holdout K``: the held-out NLPD and RMSE of the sparse ML-II plug-in (``SgprBatchResult.predict``) and,
    with ``--hmc``, of the mixture over the sparse NUTS draws (``SgprNutsResult.predict``: one launch of the batched sparse predictive
    over all draws of a cell), beside the exact ones (summary keys ``<sweep>_sparse_nlpd``, ``_sparse_rmse``, ``_sparse_hmc_nlpd``,
    ``_sparse_hmc_rmse``, one entry per cell);
  * ``--calibration`` together with ``--holdout K``: every held-out predictive also gives the mixture's 2.5 % and 97.5 % quantiles and
    its CDF at the targets (``probs=(0.025, 0.975)``: one more launch each) -- the share of held-out targets inside the central 95 %
    interval and that interval's mean width, the plug-in beside the mixture (summary keys ``<sweep>_ml2_cover95``, ``_hmc_cover95``,
    ``_ml2_width95``, ``_hmc_width95`` and, with ``--sparse M``, ``_sparse_cover95``, ``_sparse_hmc_cover95``, ``_sparse_width95``,
    ``_sparse_hmc_width95``, one entry per cell).

Writes ``<out>/hyperparameter_identification.npz`` (every fitted theta and surface) and ``.json`` (the averages the reference plots);
figures are drawn only if matplotlib imports.  ``engine`` (tests: a CPU double) defaults to the HIP engine.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggp_amd  # noqa: E402

TRUE = {"sig_sd": 5.0, "lengthscale": 2.0, "noise_sd": 1.0}
AMP_BOUNDS = (1e-5, 1e5)
CALIBRATION_PROBS = (0.025, 0.975)


def sweep(cells, n_sets, ls_upper, n_restarts, rng, latent, uniform, engine, seed, hmc=None, holdout=0, sparse=None, calibration=False):
    """cells: [(label, n_train, noise variance)].  Fits every cell with the noise fixed at its true variance and with the noise learnt.
    Returns {mode: dict(ls, sf, sn: len(cells) x n_sets, n_batches)} and the data.  ``hmc`` = dict(chains, tune, draws): also
    res["hmc"] = dict(log_ls, log_sf, log_sn: len(cells) x n_sets posterior means, diverging: the cell's share of diverging draws).
    ``holdout`` = K > 0: K more points are drawn per cell and kept out of the fit and the sampling; res["learn"] (the ML-II plug-in,
    ``Ml2Result.predict``) and res["hmc"] (the mixture over the draws, ``ExactNutsResult.predict``) gain nlpd, rmse: len(cells) x n_sets.
    ``sparse`` = dict(M, steps): also res["sparse"] = dict(ls, sf, sn, elbo: len(cells) x n_sets, seconds), the optimum of the collapsed
    bound with min(M, n) inducing inputs (it draws nothing from ``rng``); with ``hmc`` as well, res["sparse_hmc"] = dict(ls, sf, sn:
    len(cells) x n_sets posterior means of NUTS over theta at the fitted Z, diverging, seconds).  With ``holdout`` both gain nlpd, rmse
    (``SgprBatchResult.predict``, ``SgprNutsResult.predict``).  ``calibration`` (with ``holdout``): every one of these predictions is
    made with ``probs=(0.025, 0.975)`` and also gains cover95, width95: len(cells) x n_sets."""
    res = {m: {"ls": [], "sf": [], "sn": [], "lml": [], "n_batches": []} for m in ("fixed", "learn")}
    if hmc:
        res["hmc"] = {"log_ls": [], "log_sf": [], "log_sn": [], "diverging": [], "seconds": []}
    if sparse:
        res["sparse"] = {"ls": [], "sf": [], "sn": [], "elbo": [], "seconds": []}
    if sparse and hmc:
        res["sparse_hmc"] = {"ls": [], "sf": [], "sn": [], "diverging": [], "seconds": []}
    if holdout:
        for m in ("learn", "hmc", "sparse", "sparse_hmc"):
            if m in res:
                res[m].update(nlpd=[], rmse=[])
                if calibration:
                    res[m].update(cover95=[], width95=[])

    def held(r, model, X_test, Y_test):  # the held-out figures of one fitted or sampled model
        if not calibration:
            pred = model.predict(X_test, Y_test)
        else:
            pred = model.predict(X_test, Y_test, probs=CALIBRATION_PROBS)
            r["cover95"].append(pred.coverage(0.95)), r["width95"].append(pred.interval_width(0.95))
        r["nlpd"].append(pred.nlpd()), r["rmse"].append(pred.rmse(Y_test))
    data = []
    for _, n, var in cells:
        X, Y, latent = ggp_amd.identification_data(n + holdout, n_sets, rng, noise_sd=float(np.sqrt(var)), uniform=uniform, latent=latent, **{
            k: TRUE[k] for k in ("sig_sd", "lengthscale")})
        X, Y, X_test, Y_test = X[:n], Y[:, :n], X[n:], Y[:, n:]  # (the points are a random choice of the grid: any K of them are)
        data.append((X, Y))
        bounds = np.array([(1e-2, ls_upper), AMP_BOUNDS, AMP_BOUNDS])
        for mode in ("fixed", "learn"):
            fit = ggp_amd.fit_ml2(X, Y, noise=mode, theta0=[1.0, 1.0, float(var)], bounds=bounds, n_restarts=n_restarts, seed=seed,
                                  engine=engine)
            r = res[mode]
            r["ls"].append(fit.theta[:, 0]), r["sf"].append(np.sqrt(fit.theta[:, 1])), r["sn"].append(np.sqrt(fit.theta[:, 2]))
            r["lml"].append(fit.lml), r["n_batches"].append(fit.n_batches)
            if holdout and mode == "learn":
                held(r, fit, X_test, Y_test)
        if sparse:
            t0 = time.time()
            Xs = np.sort(X, 0)
            Z0 = Xs[np.round(np.linspace(0, n - 1, min(sparse["M"], n))).astype(int)]
            fit = ggp_amd.fit_sgpr_batch(X, Y, Z0, max_steps=sparse["steps"], learn_Z=True, seed=seed, engine=engine)
            r = res["sparse"]
            r["ls"].append(fit.theta[:, 0]), r["sf"].append(np.sqrt(fit.theta[:, 1])), r["sn"].append(np.sqrt(fit.theta[:, 2]))
            r["elbo"].append(fit.elbo), r["seconds"].append(time.time() - t0)
            if holdout:
                held(r, fit, X_test, Y_test)
            if hmc:
                post = fit.sample_nuts(hmc["draws"], hmc["tune"], chains=hmc["chains"], seed=seed)
                with np.errstate(invalid="ignore"):
                    mean, r = np.nanmean(np.exp(post.samples), axis=(1, 2)), res["sparse_hmc"]
                r["ls"].append(mean[:, 0]), r["sf"].append(mean[:, 1]), r["sn"].append(mean[:, 2])
                r["diverging"].append(float(np.nanmean(post.stats[..., 4]))), r["seconds"].append(post.wall_clock_secs)
                if holdout:
                    held(r, post, X_test, Y_test)
        if hmc:
            post = ggp_amd.sample_exact_nuts_batch(X, Y, hmc["draws"], hmc["tune"], chains=hmc["chains"], seed=seed, engine=engine)
            mean, r = post.posterior_mean(), res["hmc"]
            r["log_ls"].append(mean[:, 0]), r["log_sf"].append(mean[:, 1]), r["log_sn"].append(mean[:, 2])
            r["diverging"].append(float(np.nanmean(post.stats[..., 4]))), r["seconds"].append(post.wall_clock_secs)
            if holdout:
                held(r, post, X_test, Y_test)
    return {m: {k: np.array(v) for k, v in r.items()} for m, r in res.items()}, data, latent


def run(sizes=(10, 15, 20, 25, 40, 60, 80, 100, 120), noise_vars=(1, 3, 6, 9), n_sets=100, grid=50, n_noise=30, bimodal=False, seed=57,
        engine=None, hmc=None, holdout=0, sparse=None, calibration=False):
    rng = np.random.default_rng(seed)
    out, summary = {}, {"sizes": list(sizes), "noise_vars": list(noise_vars), "n_sets": n_sets, "true": TRUE}
    t0 = time.time()
    size_res, size_data, latent = sweep([(n, n, 1.0) for n in sizes], n_sets, 1e3, 10, rng, None, not bimodal, engine, seed, hmc,
                                        holdout, sparse, calibration)
    noise_res, noise_data, latent = sweep([(v, n_noise, float(v)) for v in noise_vars], n_sets, 1e4, 5, rng, latent, not bimodal, engine,
                                          seed, hmc, holdout, sparse, calibration)
    summary["fit_seconds"] = time.time() - t0
    for name, res in (("size", size_res), ("noise", noise_res)):
        for mode, r in res.items():
            for k, v in r.items():
                out["%s_%s_%s" % (name, mode, k)] = v
            if "nlpd" in r:  # held-out points: the cell's data sets averaged, the ML-II plug-in (noise learnt) beside the NUTS mixture
                tag = "ml2" if mode == "learn" else mode  # (hmc, sparse, sparse_hmc: under their own names)
                summary["%s_%s_nlpd" % (name, tag)], summary["%s_%s_rmse" % (name, tag)] = r["nlpd"].mean(1).tolist(), r["rmse"].mean(1).tolist()
                if "cover95" in r:
                    summary["%s_%s_cover95" % (name, tag)] = r["cover95"].mean(1).tolist()
                    summary["%s_%s_width95" % (name, tag)] = r["width95"].mean(1).tolist()
            if mode == "hmc":  # the posterior means of the cell's data sets, averaged; beside ML-II's log of the mean fitted lengthscale
                for k in ("log_ls", "log_sf", "log_sn"):
                    summary["%s_hmc_mean_%s" % (name, k)] = r[k].mean(1).tolist()
                summary["%s_hmc_diverging" % name], summary["%s_hmc_seconds" % name] = r["diverging"].tolist(), r["seconds"].tolist()
                continue
            if mode == "sparse_hmc":  # the sparse posterior means of the cell's data sets, averaged, beside the sparse optimum's
                summary["%s_sparse_hmc_mean_log_ls" % name] = np.log(np.nanmean(r["ls"], 1)).tolist()
                summary["%s_sparse_hmc_diverging" % name], summary["%s_sparse_hmc_seconds" % name] = r["diverging"].tolist(), r["seconds"].tolist()
                continue
            if mode == "sparse":  # beside ML-II's log of the mean fitted lengthscale: the same figure of the sparse optimum
                summary["%s_sparse_mean_log_ls" % name] = np.log(np.nanmean(r["ls"], 1)).tolist()
                summary["%s_sparse_seconds" % name] = r["seconds"].tolist()
                continue
            summary["%s_%s_mean_log_ls" % (name, mode)] = np.log(r["ls"].mean(1)).tolist()
            summary["%s_%s_batched_evaluations" % (name, mode)] = r["n_batches"].tolist()
    # surfaces: (sf2, ls) at the two smallest sizes available, noise at 1; (ls, s2) on the first noise cell with sf2 at its fit
    t0 = time.time()
    ax = np.logspace(-1, 4, grid)
    for tag, n in (("n5", 5), ("n10", 10)):
        X, Y, latent = ggp_amd.identification_data(n, 1, rng, latent=latent, **TRUE)
        out["surface_%s_X" % tag], out["surface_%s_y" % tag] = X, Y[0]
        out["surface_%s" % tag] = ggp_amd.lml_surface(X, Y[0], ax[:, None], ax[None, :], 1.0, engine=engine)  # [sf2, ls]
    Xn, Yn = noise_data[0]
    k = min(7, n_sets - 1)
    sf2_fit = float(noise_res["learn"]["sf"][0][k] ** 2)
    ax5 = np.logspace(-1, 5, grid)
    out["surface_noise"] = ggp_amd.lml_surface(Xn, Yn[k], sf2_fit, ax5[:, None], ax5[None, :], engine=engine)        # [ls, s2]
    out["surface_axis"], out["surface_noise_axis"] = ax, ax5
    summary["surface_seconds"] = time.time() - t0
    summary["surface_cells"] = int(3 * grid * grid)
    summary["surface_nan_cells"] = int(sum(np.isnan(out[k]).sum() for k in ("surface_n5", "surface_n10", "surface_noise")))
    return out, summary


def plot(out, summary, path):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    fig, axs = plt.subplots(1, 3, figsize=(13, 3.6))
    for mode, c in (("fixed", "b"), ("learn", "g")):
        axs[0].plot(summary["sizes"], summary["size_%s_mean_log_ls" % mode], c + "o-", label="noise " + mode)
        axs[1].plot(summary["noise_vars"], summary["noise_%s_mean_log_ls" % mode], c + "o-", label="noise " + mode)
    for a, lab in ((axs[0], "training set size"), (axs[1], "noise variance")):
        a.axhline(np.log(TRUE["lengthscale"]), color="r")
        a.set_xlabel(lab), a.set_ylabel("log of the mean fitted lengthscale"), a.legend(fontsize="small")
    neg = -out["surface_n10"]
    axs[2].contourf(out["surface_axis"], out["surface_axis"], np.minimum(neg, 100.0).T, levels=40)
    axs[2].set_xscale("log"), axs[2].set_yscale("log"), axs[2].set_xlabel("signal variance"), axs[2].set_ylabel("lengthscale")
    axs[2].set_title("negative LML, n = 10", fontsize="small")
    fig.tight_layout()
    fig.savefig(path, dpi=120)
    return True


def main(argv=None, engine=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10, 15, 20, 25, 40, 60, 80, 100, 120])
    ap.add_argument("--noise_vars", type=float, nargs="+", default=[1, 3, 6, 9])
    ap.add_argument("--n_sets", type=int, default=100)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--bimodal", action="store_true", help="inputs around 2 and 8 instead of uniform on the grid")
    ap.add_argument("--seed", type=int, default=57)
    ap.add_argument("--out", default="results")
    ap.add_argument("--hmc", action="store_true", help="also sample (log ls, log sig_f, log sig_n) of every data set with NUTS")
    ap.add_argument("--hmc_chains", type=int, default=4)
    ap.add_argument("--hmc_tune", type=int, default=500)
    ap.add_argument("--hmc_draws", type=int, default=500)
    ap.add_argument("--holdout", type=int, default=0, help="points per data set kept out of the fit and the sampling, and predicted")
    ap.add_argument("--calibration", action="store_true", help="with --holdout: coverage and width of the central 95 %% interval")
    ap.add_argument("--sparse", type=int, default=0, help="also fit the collapsed sparse bound with this many inducing inputs (at most 64)")
    ap.add_argument("--sparse_steps", type=int, default=2000)
    args = ap.parse_args(argv)
    if args.calibration and not args.holdout:
        ap.error("--calibration needs --holdout K")
    hmc = {"chains": args.hmc_chains, "tune": args.hmc_tune, "draws": args.hmc_draws} if args.hmc else None
    out, summary = run(args.sizes, args.noise_vars, args.n_sets, args.grid, bimodal=args.bimodal, seed=args.seed, engine=engine, hmc=hmc,
                       holdout=args.holdout, sparse={"M": args.sparse, "steps": args.sparse_steps} if args.sparse else None,
                       calibration=args.calibration)
    os.makedirs(args.out, exist_ok=True)
    base = os.path.join(args.out, "hyperparameter_identification")
    np.savez_compressed(base + ".npz", **out)
    summary["figure"] = plot(out, summary, base + ".png")
    with open(base + ".json", "w") as fh:
        json.dump(summary, fh, indent=1)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
