"""Rates of the batched device-resident NUTS over the collapsed sparse-GP bound (sgp_vfe_nuts_batch_begin / _advance: one workgroup per
chain) against the two routes the library offered before it for the same work, in the same process, the variants alternating:
aggregate leapfrogs (evaluations) per second of whole runs of C chains, C in {1, 256, 2048}, for (N, M, d) in {(200, 25, 1),
(500, 50, 1), (1000, 64, 8)} -- the shapes of profiles/vfe_batch_rates.json.  HIP events around the whole run (the begin / advance
loop and its read-backs included); one warm-up, then the median of 5.

    python tools/vfe_nuts_rates.py [--out profiles/vfe_nuts_rates.json]

The baselines: ``engine.small_nuts`` (sgp_small_nuts: one chain in one cooperative launch that occupies the chip), one chain after the
other, and the host-driven ``hmc.NUTS`` over ``vfe_eval_batch`` with P = 1 (one launch, one device-to-host copy and a Python tree
step per leapfrog).  Both run one chain at a time whatever C is, so their rate is measured on SEQ_CHAINS chains (1 for the host-driven
one) of the same batch and does not depend on C.  Chain c samples target c % N_SETS of one data set with one inducing set.  Every
shape is a child process of its own under a time limit (--cell is what the child runs); the first step that fails ends the run.  Every
row is reported, those where the batched sampler loses included.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((200, 25, 1), (500, 50, 1), (1000, 64, 8))
CS = (1, 256, 2048)
TUNE, DRAWS, DEPTH = 20, 20, 6
N_SETS, SEQ_CHAINS = 16, 4
REPS = 5
STEP_LIMIT_S = 420


def problem(N, M, d, C, seed=0):
    rng = np.random.default_rng(seed + N)
    X = rng.standard_normal((N, d))
    Y = np.sin(X.sum(1) / np.sqrt(d))[None] + 0.1 * rng.standard_normal((N_SETS, N))
    Z = X[rng.permutation(N)[:M]].copy()
    q0 = np.array([math.log(2.0)] * d + [0.0, 0.0]) + rng.uniform(-0.3, 0.3, (C, d + 2))
    seeds = [int(s) for s in rng.integers(1, 2 ** 62, C)]
    return X, Y, Z, q0, seeds


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def host_driven(eng, Xd, yd, Zd, q0, seed):
    """One chain of hmc.NUTS(rng=SplitMix(seed)) over vfe_eval_batch (P = 1) + theta_logp_and_grad.  Returns its evaluations."""
    import torch
    from ggp_amd.hmc import NUTS, DiagMassAdapter, SplitMix
    from ggp_amd.targets import in_range, theta_logp_and_grad
    nd = q0.size
    d = nd - 2

    def f(q):
        q = [float(v) for v in q]
        if not in_range(q):
            return -math.inf, [0.0] * nd
        v = [math.exp(t) for t in q]
        theta = torch.tensor([v[:d] + [v[d] * v[d], v[d + 1] * v[d + 1]]], dtype=torch.float64).to(eng.device)
        out, _, info = eng.vfe_eval_batch(Xd, yd, Zd, theta)
        row, info = out.cpu()[0].tolist(), int(info.cpu()[0])
        if info != 0 or not math.isfinite(row[0]):
            return -math.inf, [0.0] * nd
        return theta_logp_and_grad(q, v[:d], v[d], v[d + 1], row[0], row[1:1 + d], row[1 + d], row[2 + d], finite_grad=True)

    nuts = NUTS(f, nd, max_treedepth=DEPTH, rng=SplitMix(int(seed)))
    q = q0.copy()
    lp, g = nuts._eval(q)
    nuts.mass = DiagMassAdapter(nd, initial_mean=q)
    for it in range(TUNE + DRAWS):
        q, lp, g, _ = nuts.draw(q, lp, g, it < TUNE)
    return nuts.n_leapfrog


def cell(N, M, d):
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    rows = []
    for C in CS:
        X, Y, Z, q0, seeds = problem(N, M, d, C)
        Xd, Yd, Zd = T_(X), T_(Y), T_(Z)
        iy = (np.arange(C) % N_SETS).astype(np.int32)
        n_seq = min(C, SEQ_CHAINS)
        ys = [Yd[int(iy[c])].contiguous() for c in range(n_seq)]

        def batch():
            return eng.vfe_nuts_batch(Xd, Yd, Zd, q0, seeds, TUNE, DRAWS, iy=iy, max_treedepth=DEPTH)

        def sequential():
            return sum(int(eng.small_nuts(Xd, ys[c], Zd, q0[c], TUNE, DRAWS, seeds[c], max_treedepth=DEPTH)["evaluations"]) for c in range(n_seq))

        def host():
            return host_driven(eng, Xd, ys[0], Zd, q0[0], seeds[0])

        variants = [("batch", batch), ("small_nuts", sequential), ("host_driven", host)]
        for _, fn in variants:   # one warm-up each
            fn()
        torch.cuda.synchronize()
        ms, last = {k: [] for k, _ in variants}, {}
        for _ in range(REPS):    # the variants alternate
            for k, fn in variants:
                t, last[k] = event_ms(fn)
                ms[k].append(t)
        r = last["batch"]
        evals = int(r["evaluations"].sum())
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = {"N": N, "M": M, "d": d, "C": C, "reps": REPS, "tune": TUNE, "draws": DRAWS, "max_treedepth": DEPTH,
               "chains_per_cu": int(eng.vfe_nuts_lib.sgp_vfe_nuts_batch_occupancy(M, 0)),
               "evals_per_launch": int(eng.vfe_nuts_evals_per_launch(C, N, M)), "launches": int(r["launches"]),
               "bad_starts": int((r["info"] != 0).sum()), "diverging_share": float(r["stats"][:, :, 4].mean()),
               "batch_run_ms": round(med["batch"], 3), "batch_evaluations": evals,
               "batch_leapfrogs_per_s": round(evals / (med["batch"] * 1e-3), 1),
               "small_nuts_chains": n_seq, "small_nuts_leapfrogs_per_s": round(last["small_nuts"] / (med["small_nuts"] * 1e-3), 1),
               "host_driven_leapfrogs_per_s": round(last["host_driven"] / (med["host_driven"] * 1e-3), 1)}
        if C == 1:  # one chain, one workgroup: the latency of an evaluation with thread 0's sampler step
            row["batch_us_per_evaluation"] = round(1e3 * med["batch"] / evals, 2)
        row["ratio_batch_over_small_nuts"] = round(row["batch_leapfrogs_per_s"] / row["small_nuts_leapfrogs_per_s"], 3)
        row["ratio_batch_over_host_driven"] = round(row["batch_leapfrogs_per_s"] / row["host_driven_leapfrogs_per_s"], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vfe_nuts_rates.json")
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
        print(r.stdout[-3000:], flush=True)
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "baselines": "engine.small_nuts one chain after the other; hmc.NUTS over vfe_eval_batch (P = 1), host-driven",
                   "timing": "HIP events around the whole run, one warm-up, median of %d, variants alternating" % REPS,
                   "rows": rows}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
