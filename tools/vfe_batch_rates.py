"""Rates of the batched collapsed bound (sgp_vfe_eval_batch: one workgroup per problem) against the route the library offered before
it -- a loop of ``sgp_small_eval`` (one many-workgroup launch per problem) over the same problems, in the same process, the variants
alternating: microseconds per problem with gradients and value-only at P in {1, 256, 4096} for (N, M, d) in {(200, 25, 1),
(500, 50, 1), (1000, 64, 8)}.  HIP events around the enqueued work; one warm-up, then the median of 5.

    python tools/vfe_batch_rates.py [--out profiles/vfe_batch_rates.json] [--tag TEXT]

``--tag`` is recorded in the output; it names a build that differs from the product's (an A/B build with SGP_EXTRA_HIPCC_FLAGS, such as
-DSGP_AB_VFE_NO_REGISTER_BOUND -> profiles/vfe_batch_rates_no_register_bound.json).

The P problems are P rows of theta on one data set with one inducing set (dF/dZ is not requested on either side).  Every shape is a
child process of its own under a time limit (--cell is what the child runs); the first step that fails ends the run.
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

SHAPES = ((200, 25, 1), (500, 50, 1), (1000, 64, 8))
PS = (1, 256, 4096)
REPS = 5
STEP_LIMIT_S = 300


def problems(N, M, d, P, seed=0):
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.standard_normal(N)
    Z = X[rng.permutation(N)[:M]].copy()
    theta = np.exp(np.concatenate([rng.uniform(np.log(0.7), np.log(2.0), (P, d)), rng.uniform(np.log(0.5), np.log(2.0), (P, 1)),
                                   rng.uniform(np.log(0.03), np.log(0.3), (P, 1))], 1))
    return X, y, Z, theta


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cell(N, M, d):
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    lib = eng.vfe_batch_lib
    rows = []
    for P in PS:
        X, y, Z, theta = problems(N, M, d, P)
        Xd, yd, Zd, thd = T_(X), T_(y), T_(Z), T_(theta)
        out = eng.empty(P, d + 5)
        info = torch.empty(P, dtype=torch.int32, device=eng.device)
        ws = eng._workspace("vfe_batch", lib.sgp_vfe_batch_workspace_bytes(P, N, M, d, 1, 0))
        single = eng.empty(P, d + 6)   # small_eval's result rows: d + 5 values and the status word
        p = eng._ptr

        def batch(want_grad):
            st = lib.sgp_ctx_vfe_eval_batch(eng._c(), p(Xd), N * d, d, p(yd), N, None, None, p(Zd), M * d, d, None, p(thd), P, N, M, d, 0,
                                            1e-6, want_grad, p(out), None, p(info), p(ws), ws.numel(), eng._stream())
            assert st == 0

        def loop(want_grad):
            for q in range(P):
                eng.small_eval(Xd, yd, Zd, thd[q], 1e-6, want_grad=bool(want_grad), out=single[q])

        variants = [("batch_grad", lambda: batch(1)), ("loop_grad", lambda: loop(1)), ("batch_value", lambda: batch(0)),
                    ("loop_value", lambda: loop(0))]
        for _, fn in variants:   # one warm-up each
            fn()
        torch.cuda.synchronize()
        assert int((info != 0).sum()) == 0
        agree = float((out[:, 0] - single[:, 0]).abs().max() / single[:, 0].abs().max())
        ms = {k: [] for k, _ in variants}
        for _ in range(REPS):    # the variants alternate
            for k, fn in variants:
                ms[k].append(event_ms(fn))
        row = {"N": N, "M": M, "d": d, "P": P, "reps": REPS, "workgroups_per_cu": int(lib.sgp_vfe_batch_occupancy(M, 0)),
               "max_rel_F_difference": agree}
        for k in ms:
            row[k + "_us_per_problem"] = round(1e3 * statistics.median(ms[k]) / P, 3)
        row["ratio_grad_loop_over_batch"] = round(row["loop_grad_us_per_problem"] / row["batch_grad_us_per_problem"], 3)
        row["ratio_value_loop_over_batch"] = round(row["loop_value_us_per_problem"] / row["batch_value_us_per_problem"], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vfe_batch_rates.json")
    ap.add_argument("--tag", default="product build")
    ap.add_argument("--cell", help="(internal) run one shape N,M,d in this process and print its JSON line")
    a = ap.parse_args()
    if a.cell:
        print("RESULT " + json.dumps(cell(*map(int, a.cell.split(",")))), flush=True)
        return
    rows = []
    for shape in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--cell",
                            ",".join(map(str, shape))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            raise SystemExit("step %s ended with status %d: nothing more is started on the GPU" % (shape, r.returncode))
        rows += json.loads(line[0][len("RESULT "):])
        print(r.stdout[-2500:], flush=True)
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "build": a.tag, "baseline": "a loop of sgp_small_eval over the same problems",
                   "timing": "HIP events around the enqueued work, one warm-up, median of %d, variants alternating" % REPS,
                   "rows": rows}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
