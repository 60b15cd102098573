"""Rates of the batched exact-GP marginal likelihood (sgp_exact_eval_batch): microseconds per problem of the entry point alone (HIP
events, warm-up, median of --reps) at the shapes of the reference's LML surfaces and ML-II sweeps, against the only way the library
could do the same work before -- a loop of sgp_exact_eval calls on the same problems (200 of them) -- and the wall time of one whole
``fit_ml2`` at the reference's largest cell (N = 120, 100 data sets, 11 starts, noise learnt).

    python tools/exact_batch_rates.py [--reps 20] [--out profiles/exact_batch_rates.json]     # on the GPU
    python tools/exact_batch_rates.py --sklearn [--out ...]                                   # on the CPU: scikit-learn's time

Every GPU step is a child process of its own under a time limit (--cell NAME is what the child runs); the first step that fails ends
the run.  Results are merged into --out, so the scikit-learn figure (CPU seconds of the machine it ran on) and the GPU figures may
come from two runs.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, P, with_grad)
BATCH = [(5, 10000, 0), (30, 10000, 0), (120, 2500, 0), (120, 1100, 1), (128, 1100, 1)]
LOOP = 200
FIT = {"N": 120, "n_sets": 100, "n_restarts": 10, "noise": "learn"}
BOUNDS = np.array([(1e-2, 1e3), (1e-5, 1e5), (1e-5, 1e5)])
STEP_LIMIT_S = 240


def problems(N, P, seed=0):
    """One data set of the identification study at N points and P hyper-parameter rows, log-uniform over the surfaces' ranges."""
    import ggp_amd
    rng = np.random.default_rng(seed)
    X, Y, _ = ggp_amd.identification_data(N, 1, rng)
    theta = np.exp(np.stack([rng.uniform(np.log(0.1), np.log(1e2), P), rng.uniform(np.log(0.1), np.log(1e4), P),
                             rng.uniform(np.log(0.1), np.log(1e2), P)], 1))
    return X, Y[0], theta


def timed(fn, reps, warm=3):
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
    return statistics.median(ms)


def cell_batch(N, P, wg, reps):
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    lib = eng.lib
    X, y, theta = problems(N, P)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    Xd, yd, thd = T(X), T(y), T(theta)
    d = X.shape[1]
    out, grads = eng.empty(P, 4), eng.empty(P, d + 2)
    info = torch.empty(P, dtype=torch.int32, device=eng.device)
    ws = eng._workspace("exact_batch", lib.sgp_exact_batch_workspace_bytes(P, N, d, wg))

    def batch():  # the entry point alone
        st = lib.sgp_ctx_exact_eval_batch(eng._c(), eng._ptr(Xd), N * d, d, eng._ptr(yd), N, None, None, eng._ptr(thd), P, N, d, 0, wg,
                                          eng._ptr(out), eng._ptr(grads), eng._ptr(info), eng._ptr(ws), ws.numel(), eng._stream())
        assert st == 0

    ms = timed(batch, reps)
    n_bad = int((info != 0).sum())
    # the loop: the first LOOP problems through sgp_exact_eval, entry point alone as well (no host copy per call)
    H = eng.EXACT_HEAD
    buf = eng.empty(H + d + 2)
    info1 = buf[4:5].view(torch.int32)[:1]
    ws1 = eng._workspace("exact", lib.sgp_exact_workspace_bytes(N, d, 1))
    rows = [((C.c_double * d)(*[1.0 / v for v in theta[p, :d]]), float(theta[p, d]), float(theta[p, d + 1])) for p in range(LOOP)]

    def loop():
        for ils, sf2, s2 in rows:
            st = lib.sgp_ctx_exact_eval(eng._c(), eng._ptr(Xd), d, eng._ptr(yd), N, d, ils, sf2, s2, 0, wg, C.c_void_p(buf.data_ptr()),
                                        C.c_void_p(buf.data_ptr() + 8 * H), None, eng._ptr(info1), eng._ptr(ws1), ws1.numel(),
                                        eng._stream())
            assert st == 0

    loop_ms = timed(loop, reps)
    return {"N": N, "P": P, "with_grad": wg, "reps": reps, "batch_ms": round(ms, 4), "batch_us_per_problem": round(1e3 * ms / P, 4),
            "loop_us_per_problem": round(1e3 * loop_ms / LOOP, 3), "loop_over_batch": round((loop_ms / LOOP) / (ms / P), 1),
            "workgroups_per_cu": int(lib.sgp_exact_batch_occupancy(N, 0)), "problems_not_pd": n_bad}


def fit_data():
    import ggp_amd
    return ggp_amd.identification_data(FIT["N"], FIT["n_sets"], np.random.default_rng(57))[:2]


def cell_fit():
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    X, Y = fit_data()
    kw = dict(noise=FIT["noise"], theta0=[1.0, 1.0, 1.0], bounds=BOUNDS, n_restarts=FIT["n_restarts"], seed=0, engine=eng)
    ggp_amd.fit_ml2(X, Y[:2], **kw)  # warm-up: library, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ggp_amd.fit_ml2(X, Y, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(FIT, fit_ml2_wall_s=round(wall, 3), batched_evaluations=int(res.n_batches), starts_converged=int(res.converged.sum()),
                starts=int(res.converged.size), mean_lml=float(res.lml.mean()), mean_log_ls=float(np.log(res.theta[:, 0]).mean()))


def sklearn_cpu(n_sets=10):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    X, Y = fit_data()
    t0 = time.perf_counter()
    lml = []
    for b in range(n_sets):
        k = ConstantKernel(1.0, tuple(BOUNDS[1])) * RBF(1.0, tuple(BOUNDS[0])) + WhiteKernel(1.0, tuple(BOUNDS[2]))
        gp = GaussianProcessRegressor(kernel=k, alpha=0.0, n_restarts_optimizer=FIT["n_restarts"], random_state=b).fit(X, Y[b])
        lml.append(gp.log_marginal_likelihood_value_)
    wall = time.perf_counter() - t0
    return {"N": FIT["N"], "n_sets": n_sets, "n_restarts": FIT["n_restarts"], "cpu_wall_s": round(wall, 3),
            "cpu_s_per_data_set": round(wall / n_sets, 3), "mean_lml": float(np.mean(lml)),
            "note": "CPU seconds of the machine this ran on (scikit-learn + scipy L-BFGS-B), not a GPU figure"}


def merge(path, update):
    res = {}
    if os.path.exists(path):
        with open(path) as fh:
            res = json.load(fh)
    res.update(update)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/exact_batch_rates.json")
    ap.add_argument("--sklearn", action="store_true", help="time scikit-learn on 10 of the fit's data sets (CPU) and merge it into --out")
    ap.add_argument("--cell", help="(internal) run one step in this process and print its JSON line")
    a = ap.parse_args()
    if a.cell:
        kind, *rest = a.cell.split(":")
        row = cell_fit() if kind == "fit" else cell_batch(*[int(v) for v in rest], reps=a.reps)
        print("RESULT " + json.dumps(row), flush=True)
        return
    if a.sklearn:
        merge(a.out, {"sklearn_cpu": sklearn_cpu()})
        return
    rows, fit = [], None
    for name in ["batch:%d:%d:%d" % c for c in BATCH] + ["fit"]:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--cell", name,
                            "--reps", str(a.reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            raise SystemExit("step %s ended with status %d: nothing more is started on the GPU" % (name, r.returncode))
        row = json.loads(line[0][len("RESULT "):])
        print(json.dumps(row), flush=True)
        if name == "fit":
            fit = row
        else:
            rows.append(row)
    import torch
    merge(a.out, {"device": torch.cuda.get_device_name(0), "reps": a.reps, "loop_problems": LOOP, "batched": rows, "fit_ml2": fit})


if __name__ == "__main__":
    main()
