"""Rates of the batched exact-GP predictive (sgp_exact_predict_batch + sgp_exact_mixture_reduce): microseconds per draw of the two
entry points alone (HIP events around both launches, warm-up, median and quartiles of --reps), against the per-draw loop the library
offered before -- ``exact_eval(want_factors=True)`` + ``exact_predict`` + the read of ``info``, the device work of
``models._mixture_loop`` -- over N in {32, 64, 128} x T in {100, 500} x P in {1, 256, 65 536} draws.

    python tools/exact_predict_rates.py [--reps 20] [--what both|batch|loop] [--tag NAME] [--out profiles/exact_predict_rates.json]

The loop costs the same per draw whatever P is: it is timed over min(P, 64) draws per repetition.  ``--what loop`` needs nothing of
the batched path, so the same script times the loop on a commit that does not have it yet (``--tag`` names the commit in the output:
rows are merged into --out under "loop" with their tag, the batched rows under "batched").  Every N is a child process of its own under
a time limit (--cell N is what the child runs); the first step that fails ends the run.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS, TS, PS = (32, 64, 128), (100, 500), (1, 256, 65536)
LOOP_DRAWS = 64
GROUP = 256  # draws per group of the mixture (a data set's chains x draws)
STEP_LIMIT_S = 400


def problems(N, T, P, seed=0):
    """One data set of the identification study at N points, T test points of [0, 10], and P hyper-parameter rows over the range its
    posteriors cover."""
    import ggp_amd
    rng = np.random.default_rng(seed)
    X, Y, _ = ggp_amd.identification_data(N, 1, rng)
    Xs = rng.uniform(0.0, 10.0, (T, 1))
    theta = np.exp(np.stack([rng.uniform(np.log(0.5), np.log(5.0), P), rng.uniform(np.log(1.0), np.log(50.0), P),
                             rng.uniform(np.log(0.3), np.log(3.0), P)], 1))
    return X, Y[0], Xs, theta, rng.standard_normal((-(-P // GROUP), T))


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


def cell(N, reps, what):
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    rows = []
    for T in TS:
        for P in PS:
            X, y, Xs, theta, Yt = problems(N, T, P)
            Xd, yd, Xsd, thd, Ytd = T_(X), T_(y), T_(Xs), T_(theta), T_(Yt)
            d = X.shape[1]
            row = {"N": N, "T": T, "P": P, "reps": reps}
            if what in ("both", "batch"):
                lib = eng.exact_predict_lib
                G = Yt.shape[0]
                off = torch.as_tensor(np.minimum(np.arange(G + 1) * GROUP, P), dtype=torch.int64).to(eng.device)
                mean, var = eng.empty(P, T), eng.empty(P, T)
                info = torch.empty(P, dtype=torch.int32, device=eng.device)
                mix = [eng.empty(G, T) for _ in range(4)]
                kept = torch.empty(G, dtype=torch.int32, device=eng.device)
                ws = eng._workspace("exact_predict_batch", lib.sgp_exact_predict_batch_workspace_bytes(P, N, d, T))
                p = eng._ptr

                def batch():  # the two entry points alone
                    st = lib.sgp_ctx_exact_predict_batch(eng._c(), p(Xd), N * d, d, p(yd), N, p(Xsd), T * d, d, T, None, None, None, p(thd),
                                                         P, N, d, 0, 1, p(mean), p(var), p(info), p(ws), ws.numel(), eng._stream())
                    assert st == 0
                    st = lib.sgp_exact_mixture_reduce(p(mean), p(var), p(info), p(off), G, T, p(Ytd), p(mix[0]), p(mix[1]), p(mix[2]),
                                                      p(mix[3]), p(kept), p(ws), ws.numel(), eng._stream())
                    assert st == 0

                ms, lo, hi = timed(batch, reps)
                assert int((info != 0).sum()) == 0 and int(kept.sum()) == P and bool(mix[2].isfinite().all())
                row.update(batch_ms=round(ms, 4), batch_us_per_draw=round(1e3 * ms / P, 4),
                           batch_us_per_draw_quartiles=[round(1e3 * lo / P, 4), round(1e3 * hi / P, 4)],
                           workgroups_per_cu=int(lib.sgp_exact_predict_batch_occupancy(N, 0)))
            if what in ("both", "loop"):
                n = min(P, LOOP_DRAWS)
                draws = [(list(theta[s, :d]), float(theta[s, d]), float(theta[s, d + 1])) for s in range(n)]

                def loop():  # per draw: the factors (its host copy of `out` is the read of info), then the predictive
                    for ls, sf2, s2 in draws:
                        r = eng.exact_eval(Xd, yd, ls, sf2, s2, want_grad=False, want_factors=True)
                        assert r["info"] == 0
                        eng.exact_predict(Xsd, Xd, ls, sf2, s2, r["factors"], pred_noise=True)

                ms, lo, hi = timed(loop, reps)
                row.update(loop_draws=n, loop_us_per_draw=round(1e3 * ms / n, 2),
                           loop_us_per_draw_quartiles=[round(1e3 * lo / n, 2), round(1e3 * hi / n, 2)])
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def merge(path, batched, loop, tag, head):
    res = {}
    if os.path.exists(path):
        with open(path) as fh:
            res = json.load(fh)
    res.update(head)
    if batched:
        res["batched"] = batched
    if loop:
        res.setdefault("loop", {})[tag] = loop
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--what", choices=("both", "batch", "loop"), default="both")
    ap.add_argument("--tag", default="this commit", help="names the commit the loop was timed on")
    ap.add_argument("--out", default="profiles/exact_predict_rates.json")
    ap.add_argument("--cell", type=int, help="(internal) run one N in this process and print its JSON line")
    a = ap.parse_args()
    if a.cell:
        print("RESULT " + json.dumps(cell(a.cell, a.reps, a.what)), flush=True)
        return
    rows = []
    for N in NS:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--cell", str(N),
                            "--reps", str(a.reps), "--what", a.what], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            raise SystemExit("step N = %d ended with status %d: nothing more is started on the GPU" % (N, r.returncode))
        rows += json.loads(line[0][len("RESULT "):])
        print(r.stdout[-2500:], flush=True)
    import torch
    keys_b = ("N", "T", "P", "reps", "batch_ms", "batch_us_per_draw", "batch_us_per_draw_quartiles", "workgroups_per_cu")
    keys_l = ("N", "T", "P", "reps", "loop_draws", "loop_us_per_draw", "loop_us_per_draw_quartiles")
    batched = [{k: r[k] for k in keys_b} for r in rows] if a.what != "loop" else None
    loop = [{k: r[k] for k in keys_l} for r in rows] if a.what != "batch" else None
    merge(a.out, batched, loop, a.tag, {"device": torch.cuda.get_device_name(0), "group_draws": GROUP})


if __name__ == "__main__":
    main()
