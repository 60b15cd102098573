"""Rates of the multi-class (robust-max) SVGP bound: device ms per bound and per bound + gradient of ``HipEngine.svgp_mc_elbo`` for C in
{3, 10} beside the existing Bernoulli chain (``svgp_elbo_batch`` with one hyper-parameter sample) at the same shape, in the same run --
the Bernoulli chain is the yardstick; the ratio is reported, not asserted -- and the number of kernel launches of one step with
gradients for C = 3 and C = 10, which must be the same.

One process for the timings; warm-up first; HIP events on the stream around every timed call (nothing synchronises inside the bracket:
the events span the device's work on the chain as the host enqueues it); the variants ALTERNATE (a, b, c, a, b, c, ...) so that clock
drift hits all alike; median and quartiles of 20 repetitions.  Shapes (B, M, d): (4096, 256, 2), the minibatch of the C4 workload, and
(200, 100, 8).

The launch counts come from kernel-trace runs of their own: this script starts itself as a child under ``rocprofv3 --kernel-trace`` with
``--trace-steps n`` for n = 2 and n = 4 and takes (rows(4) - rows(2)) / 2 of the trace, so that start-up work cancels; the count of
kernels of the library (names in namespace ``sgp``) is given beside the count of all dispatches (torch's fills of the result buffers).

    python tools/svgp_mc_rates.py [--reps 20] [--out profiles/svgp_mc_rates.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ggp_amd  # noqa: E402

SHAPES = [(4096, 256, 2), (200, 100, 8)]
CLASSES = (3, 10)
TRACE_SHAPE = SHAPES[0]
JITTER = 1e-6
# passes over the Mp x Bp block A and the C blocks T_c per step with gradients
PASSES = {"A": "read 6 times whatever C is: T (batched product), cols, g_m, abar, G (batched product), S1",
          "T_c": "each class's block written twice (T, the scaling in place) and read 4 times (cols, scaling, W, G)"}


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


def alternate(fns, reps, warm=3):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    acc = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, acc):
            t.append(timed(fn))
    return acc


def problem(eng, B, M, d, C, seed=0):
    """Inputs on the device: X uniform, Z a subset of its rows, q(u_c) near the prior, labels uniform over the classes."""
    rng = np.random.default_rng(seed + 101 * C)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(eng.device)  # noqa: E731
    X = rng.uniform(-2.0, 2.0, (B, d))
    Z = X[rng.permutation(B)[:M]] + 0.01 * rng.standard_normal((M, d))
    m = 0.3 * rng.standard_normal((C, M))
    LS = np.tril(0.05 * rng.standard_normal((C, M, M)), -1) + np.eye(M)
    y = rng.integers(0, C, B).astype(np.float64)
    return dict(X=dev(X), y=dev(y), Z=dev(Z), m=dev(m), LS=dev(LS), ls=[0.8] * d, sf2=1.2, N=100000)


def mc_step(eng, p, grads):
    return eng.svgp_mc_elbo(p["X"], p["y"], p["Z"], p["ls"], p["sf2"], p["m"], p["LS"], p["N"], jitter=JITTER, with_grads=grads)


def bernoulli_step(eng, p, grads):
    return eng.svgp_elbo_batch(p["X"], p["yb"], p["Z"], [p["ls"]], [p["sf2"]], [1.0], p["m"][0], p["LS"][0], p["N"], jitter=JITTER,
                               likelihood="bernoulli", with_grads=grads)


def trace_child(C, steps):
    eng = ggp_amd.HipEngine(torch.device("cuda", 0))
    p = problem(eng, *TRACE_SHAPE, C)
    for _ in range(steps):
        mc_step(eng, p, True)
    torch.cuda.synchronize()


def trace_rows(C, steps):
    """(all dispatches, dispatches of kernels in namespace sgp) of a child that runs ``steps`` steps under a kernel trace."""
    out = tempfile.mkdtemp(prefix="svgp_mc_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--trace-steps", str(steps), "--trace-classes", str(C)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("kernel-trace child failed (%d): %s" % (r.returncode, r.stdout[-500:]))
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel trace written: %s" % r.stdout[-500:])
        total = lib = 0
        for f in files:
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    total += 1
                    name = row.get("Kernel_Name", "")
                    lib += "sgp::" in name or "N3sgp" in name  # demangled or not
        return total, lib
    finally:
        shutil.rmtree(out, ignore_errors=True)


def launch_counts():
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    res = {}
    for C in CLASSES:
        try:
            (t2, l2), (t4, l4) = trace_rows(C, 2), trace_rows(C, 4)
            res["C=%d" % C] = {"library_kernels_per_step": (l4 - l2) / 2, "all_dispatches_per_step": (t4 - t2) / 2,
                               "trace_rows": {"2 steps": [t2, l2], "4 steps": [t4, l4]}}
        except Exception as e:  # the timings above stand without the trace
            res["C=%d" % C] = {"error": str(e)}
    counts = [v.get("library_kernels_per_step") for v in res.values()]
    res["same_for_all_C"] = None if None in counts else len(set(counts)) == 1
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/svgp_mc_rates.json")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--trace-classes", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.trace_steps:
        trace_child(args.trace_classes, args.trace_steps)
        return
    eng = ggp_amd.HipEngine(torch.device("cuda", 0))
    rec = {"tool": "tools/svgp_mc_rates.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "passes": PASSES, "shapes": []}
    for B, M, d in SHAPES:
        probs = {C: problem(eng, B, M, d, C) for C in CLASSES}
        pb = dict(probs[CLASSES[0]])
        pb["yb"] = torch.where(pb["y"] > 0, torch.ones_like(pb["y"]), -torch.ones_like(pb["y"]))
        names, fns = [], []
        for grads in (False, True):
            names.append(("bernoulli_S1", grads))
            fns.append(lambda g=grads: bernoulli_step(eng, pb, g))
            for C in CLASSES:
                names.append(("multiclass_C%d" % C, grads))
                fns.append(lambda g=grads, c=C: mc_step(eng, probs[c], g))
        acc = alternate(fns, args.reps)
        entry = {"B": B, "M": M, "d": d, "ms": {}}
        for (name, grads), ms in zip(names, acc):
            entry["ms"].setdefault(name, {})["bound_and_gradient" if grads else "bound"] = spread(ms)
        base = entry["ms"]["bernoulli_S1"]
        for C in CLASSES:
            e = entry["ms"]["multiclass_C%d" % C]
            e["ratio_to_bernoulli"] = {k: round(e[k]["median"] / base[k]["median"], 3) for k in ("bound", "bound_and_gradient")}
        rec["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    rec["launches_per_step_with_gradients"] = {"shape": list(TRACE_SHAPE)} if args.no_trace else dict(launch_counts(), shape=list(TRACE_SHAPE))
    print(json.dumps(rec["launches_per_step_with_gradients"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
