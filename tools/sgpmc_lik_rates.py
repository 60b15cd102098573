"""Rates of SGPMC with a non-conjugate likelihood: device ms per value and per value + gradient of ``SgpmcTarget(likelihood=...)``
for the Poisson and the Bernoulli (probit) likelihood beside the existing Gaussian ``SgpmcTarget`` at the same shape, in the same call.

One process; warm-up first; HIP events on the stream around every timed call (the host side of an evaluation -- one device-to-host
copy -- is inside the bracket, as a sampler sees it); the targets ALTERNATE (a, b, c, a, b, c, ...) so that clock drift hits all
alike; median and quartiles are recorded.  The big shapes are the ones the test-suite's long-double reference cannot reach (tapered
contraction splits, several rounds of workgroups), so every shape is also CHECKED: dmu and dv of a row subsample against the CPU
restatement of csrc/sgp_lik.hpp in torch fp64, and G against sf2^2 (T diag(dv))^T T formed by torch.matmul on the device from the
value-only call's T.

    python tools/sgpmc_lik_rates.py [--reps 10] [--shapes c4,c5] [--out profiles/sgpmc_lik_rates.json]
    rocprofv3 --kernel-trace --stats -- python tools/sgpmc_lik_rates.py --shapes c5 --liks poisson --reps 3   (the two new kernels alone:
                                                                                         a run of its own, one likelihood at a time)
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ggp_amd  # noqa: E402

SHAPES = {"c4": ("C4 shape", 100_000, 2, 256), "c5": ("C5 shape", 1_000_000, 8, 1024), "tiny": ("tiny", 5000, 2, 64)}
JITTER = 1e-5
HBM_ACHIEVABLE = 6.3e12   # bytes / s


def problem(N, d, M, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    f = np.sin(2.0 * X @ w)
    return X, f, X[rng.choice(N, M, replace=False)].copy(), rng


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median": round(statistics.median(ms), 4), "q1": round(q[0], 4), "q3": round(q[2], 4), "reps": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warm=2):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, acc):
            t.append(timed(fn))
    return acc


def check(eng, tgt, q, lik):
    """(worst relative error of dmu, dv on a row subsample against the CPU restatement, relative error of G against torch.matmul)"""
    from sgpmc_lik_double import LIK, lik_terms
    d, M, N = tgt.d, tgt.M, tgt.N
    sp = lambda x: x + math.log1p(math.exp(-x)) if x > 0 else math.log1p(math.exp(x))
    sf2, ls = sp(q[0]), [sp(t) for t in q[1:1 + d]]
    v = torch.tensor(q[tgt.n_theta:], dtype=torch.float64, device=eng.device)
    linv, _ = eng.kuu_factor(eng.kuu(tgt.Z, ls, sf2, JITTER, "rbf"))
    t = eng.kfu_buffer(N, M)
    val = eng.sgpmc_lik_rows(tgt.X, tgt.y, tgt.Z, ls, sf2, 1.0, v, linv, t, "rbf", lik, want_adjoints=False)
    Mp = (M + 127) // 128 * 128
    T = t[: ((N + 255) // 256 * 256) * Mp].reshape(-1, Mp)[:N, :M].clone()
    full = eng.sgpmc_lik_rows(tgt.X, tgt.y, tgt.Z, ls, sf2, 1.0, v, linv, t, "rbf", lik, want_adjoints=True)
    assert torch.equal(val["out"], full["out"]) and torch.equal(val["dv"], full["dv"])
    G = (sf2 * sf2) * (T * full["dv"][:, None]).T @ T
    err_G = float((full["G"] - G).abs().max() / G.abs().max())
    g = sf2 * (T.T @ full["dmu"])
    err_g = float((full["g"] - g).abs().max() / g.abs().max())
    rows = torch.arange(0, N, max(1, N // 2000), device=eng.device)
    a = (sf2 * T[rows]).cpu()
    mu, var = a @ v.cpu(), sf2 - (a * a).sum(1)
    _, dmu, dv, _ = lik_terms(LIK[lik], tgt.y[rows].cpu(), mu, var, 1.0)
    e = lambda got, want: float((got.cpu() - want).abs().max() / want.abs().max())
    return {"rows_checked": int(rows.numel()), "rel_err_dmu": e(full["dmu"][rows], dmu), "rel_err_dv": e(full["dv"][rows], dv),
            "rel_err_G_vs_matmul": err_G, "rel_err_g_vs_matmul": err_g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="c4,c5")
    ap.add_argument("--out", default="profiles/sgpmc_lik_rates.json")
    ap.add_argument("--liks", default="gaussian,poisson,bernoulli", help="targets to run (a profiler run takes one new likelihood at a time)")
    a = ap.parse_args()
    eng = ggp_amd.HipEngine()
    D = lambda t: torch.as_tensor(t, dtype=torch.float64, device=eng.device).contiguous()
    sp_inv = lambda c: c + math.log(-math.expm1(-c))
    out = []
    for key in a.shapes.split(","):
        name, N, d, M = SHAPES[key]
        X, f, Z, rng = problem(N, d, M)
        ys = {"gaussian": f + 0.1 * rng.standard_normal(N), "poisson": rng.poisson(np.exp(f)).astype(np.float64),
              "bernoulli": np.where(f + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0)}
        Xd, Zd = D(X), D(Z)
        ls, sf2 = [math.sqrt(d) * 1.2] * d, 1.0
        vq = list(0.5 * rng.standard_normal(M))
        tg, qs = {}, {}
        for lik in a.liks.split(","):
            tg[lik] = ggp_amd.SgpmcTarget(Xd, D(ys[lik]), Zd, jitter=JITTER, engine=eng, likelihood=lik)
            tg[lik].whitened_rows_min_work = 0      # the Gaussian target in the same rows layout at every shape
            qs[lik] = np.array([sp_inv(sf2)] + [sp_inv(t) for t in ls] + ([sp_inv(0.1 - 1e-6)] if lik == "gaussian" else []) + vq)
        liks = list(tg)
        for lik in liks:
            lp, g = tg[lik].logp_and_grad(qs[lik])
            assert math.isfinite(lp) and all(math.isfinite(t) for t in g), (lik, lp)
        val = alternate([lambda l=l: tg[l].logp(qs[l]) for l in liks], a.reps)
        grd = alternate([lambda l=l: tg[l].logp_and_grad(qs[l]) for l in liks], a.reps)
        row = {"shape": name, "N": N, "d": d, "M": M}
        for i, lik in enumerate(liks):
            row["ms_value_" + lik], row["ms_value_and_grad_" + lik] = spread(val[i]), spread(grd[i])
        for lik in [l for l in liks if l != "gaussian"]:
            if "gaussian" in liks:
                ig, il = liks.index("gaussian"), liks.index(lik)
                row["gaussian_pass1"] = tg["gaussian"].last_pass1
                row["ratio_value_%s_over_gaussian" % lik] = round(statistics.median(val[il]) / statistics.median(val[ig]), 4)
                row["ratio_value_and_grad_%s_over_gaussian" % lik] = round(statistics.median(grd[il]) / statistics.median(grd[ig]), 4)
            row["check_" + lik] = check(eng, tg[lik], qs[lik], lik)
        Np, Mp = (N + 255) // 256 * 256, (M + 127) // 128 * 128
        row["bytes_per_pass_over_T"] = 8 * Np * Mp
        row["ms_per_pass_over_T_at_hbm_achievable"] = round(8 * Np * Mp / HBM_ACHIEVABLE * 1e3, 4)
        out.append(row)
        print(json.dumps(row), flush=True)
        del tg, Xd, Zd
        eng._ws.clear()
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "measured_on_gpu": True, "reps": a.reps, "rates": out}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
