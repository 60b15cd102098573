"""Rates of the batched sparse-GP predictive (sgp_vfe_predict_batch + sgp_exact_mixture_reduce): microseconds per draw of the two entry
points alone (HIP events around both launches, three warm-up runs, median and quartiles of --reps), against the route the library
offered before -- ``HipEngine.mixture_predict(..., full_cov=False)`` for one data set, eight draws per chain of launches, with the host
copy of its status -- at the shapes (N, M, d, T) of profiles/vfe_nuts_rates.json and P in {1, 256, 4096} draws in groups of 256.

    python tools/vfe_predict_rates.py [--reps 20] [--what both|batch|route] [--tag NAME] [--out profiles/vfe_predict_rates.json]

The route costs the same per draw whatever P is: it is timed over min(P, 64) draws per repetition.  ``--what route`` needs nothing of
the batched path, so the same script times the route on a commit that does not have it yet (``--tag`` names the commit in the output:
rows are merged into --out under "route" with their tag, the batched rows under "batched").  With both in one run every row also
carries the ratio of the medians and ``wins``: the batched median lies below the route's by more than the two inter-quartile ranges
added together.  Every shape is a child process of its own under a time limit (--cell I is what the child runs); the first step that
fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((200, 25, 1, 100), (500, 50, 1, 500), (1000, 64, 8, 500))   # (N, M, d, T)
PS = (1, 256, 4096)
ROUTE_DRAWS = 64
GROUP = 256  # draws per group of the mixture (a data set's chains x draws)
STEP_LIMIT_S = 400
JITTER = 1e-6


def problems(N, M, d, T, P, seed=0):
    """One data set (X standard normal, y a smooth function of it plus noise, Z a random subset of X), T test points and P
    hyper-parameter rows [ls | sf2 | s2] over the range a posterior of such a data set covers."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.standard_normal(N)
    Z = X[rng.permutation(N)[:M]].copy()
    Xs = 1.5 * rng.standard_normal((T, d))
    theta = np.exp(np.concatenate([rng.uniform(np.log(0.7), np.log(1.5), (P, d)), rng.uniform(np.log(0.5), np.log(2.0), (P, 1)),
                                   rng.uniform(np.log(0.03), np.log(0.3), (P, 1))], 1))
    return X, y, Z, Xs, theta, rng.standard_normal((-(-P // GROUP), T))


def timed(fn, reps, warm=3):
    """(median, lower quartile, upper quartile) of the milliseconds of fn between two events on the current stream."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), q[0], q[2]


def cell(shape, reps, what):
    import torch
    import ggp_amd
    N, M, d, T = shape
    eng = ggp_amd.HipEngine()
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    rows = []
    for P in PS:
        X, y, Z, Xs, theta, Yt = problems(N, M, d, T, P)
        Xd, yd, Zd, Xsd, thd, Ytd = T_(X), T_(y), T_(Z), T_(Xs), T_(theta), T_(Yt)
        row = {"N": N, "M": M, "d": d, "T": T, "P": P, "reps": reps}
        if what in ("both", "batch"):
            lib, mix_lib = eng.vfe_predict_lib, eng.exact_predict_lib
            G = Yt.shape[0]
            off = torch.as_tensor(np.minimum(np.arange(G + 1) * GROUP, P), dtype=torch.int64).to(eng.device)
            mean, var, bound = eng.empty(P, T), eng.empty(P, T), eng.empty(P)
            info = torch.empty(P, dtype=torch.int32, device=eng.device)
            mix = [eng.empty(G, T) for _ in range(4)]
            kept = torch.empty(G, dtype=torch.int32, device=eng.device)
            ws = eng._workspace("vfe_predict", lib.sgp_vfe_predict_batch_workspace_bytes(P, N, M, d, T))
            p = eng._ptr

            def batch():  # the two entry points alone
                st = lib.sgp_ctx_vfe_predict_batch(eng._c(), p(Xd), N * d, d, p(yd), N, None, None, p(Zd), M * d, d, None, p(Xsd), T * d, d,
                                                   T, None, p(thd), P, N, M, d, 0, JITTER, 1, p(mean), p(var), p(bound), p(info), p(ws),
                                                   ws.numel(), eng._stream())
                assert st == 0
                st = mix_lib.sgp_exact_mixture_reduce(p(mean), p(var), p(info), p(off), G, T, p(Ytd), p(mix[0]), p(mix[1]), p(mix[2]),
                                                      p(mix[3]), p(kept), p(ws), ws.numel(), eng._stream())
                assert st == 0

            ms, lo, hi = timed(batch, reps)
            assert int((info != 0).sum()) == 0 and int(kept.sum()) == P and bool(mix[2].isfinite().all()) and bool(bound.isfinite().all())
            row.update(batch_ms=round(ms, 4), batch_us_per_draw=round(1e3 * ms / P, 4),
                       batch_us_per_draw_quartiles=[round(1e3 * lo / P, 4), round(1e3 * hi / P, 4)],
                       workgroups_per_cu=int(lib.sgp_vfe_predict_batch_occupancy(M, 0)))
        if what in ("both", "route"):
            n = min(P, ROUTE_DRAWS)
            ls, sf2, s2 = theta[:n, :d].tolist(), theta[:n, d].tolist(), theta[:n, d + 1].tolist()

            def route():  # one data set: eight draws per chain of launches, then the host copy of the status
                r = eng.mixture_predict(Xd, yd, Xsd, Zd, ls, sf2, s2, jitter=JITTER, kernel="rbf", pred_noise=True, full_cov=False)
                assert int(r["info"].cpu().abs().sum()) == 0

            ms, lo, hi = timed(route, reps)
            row.update(route_draws=n, route_us_per_draw=round(1e3 * ms / n, 2),
                       route_us_per_draw_quartiles=[round(1e3 * lo / n, 2), round(1e3 * hi / n, 2)])
        if what == "both":
            b, r = row["batch_us_per_draw_quartiles"], row["route_us_per_draw_quartiles"]
            row["route_over_batch"] = round(row["route_us_per_draw"] / row["batch_us_per_draw"], 2)
            row["wins"] = bool(row["batch_us_per_draw"] < row["route_us_per_draw"] - ((b[1] - b[0]) + (r[1] - r[0])))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def merge(path, batched, route, tag, head):
    res = {}
    if os.path.exists(path):
        with open(path) as fh:
            res = json.load(fh)
    res.update(head)
    if batched:
        res["batched"] = batched
    if route:
        res.setdefault("route", {})[tag] = route
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--what", choices=("both", "batch", "route"), default="both")
    ap.add_argument("--tag", default="this commit", help="names the commit the route was timed on")
    ap.add_argument("--out", default="profiles/vfe_predict_rates.json")
    ap.add_argument("--cell", type=int, default=-1, help="(internal) run shape number I in this process and print its JSON line")
    a = ap.parse_args()
    if a.cell >= 0:
        print("RESULT " + json.dumps(cell(SHAPES[a.cell], a.reps, a.what)), flush=True)
        return
    rows = []
    for i, shape in enumerate(SHAPES):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--cell", str(i),
                            "--reps", str(a.reps), "--what", a.what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            raise SystemExit("step %s ended with status %d: nothing more is started on the GPU" % (shape, r.returncode))
        rows += json.loads(line[0][len("RESULT "):])
        print(r.stdout[-2500:], flush=True)
    import torch
    head_keys = ("N", "M", "d", "T", "P", "reps")
    keys_b = head_keys + ("batch_ms", "batch_us_per_draw", "batch_us_per_draw_quartiles", "workgroups_per_cu") + \
        (("route_over_batch", "wins") if a.what == "both" else ())
    keys_r = head_keys + ("route_draws", "route_us_per_draw", "route_us_per_draw_quartiles")
    batched = [{k: r[k] for k in keys_b} for r in rows] if a.what != "route" else None
    route = [{k: r[k] for k in keys_r} for r in rows] if a.what != "batch" else None
    merge(a.out, batched, route, a.tag, {"device": torch.cuda.get_device_name(0), "group_draws": GROUP, "jitter": JITTER})


if __name__ == "__main__":
    main()
