"""Rates of the batched device-resident NUTS over the exact GP (sgp_exact_nuts_batch_begin / _advance): leapfrogs (evaluations) per
second of whole runs of C chains, C in {1, 256, 2048}, on data sets of the identification study at N in {20, 64, 128} (HIP events
around the begin / advance loop, one warm-up run, median of --reps), the time per evaluation of ONE chain (the C = 1 cells: what the
default of ``evals_per_launch`` is chosen from) and, as the baseline from the same box and the same data, the host-driven
``sample_nuts(ExactHmcTarget)``: one ``sgp_exact_eval``, one device-to-host copy and a Python tree step per leapfrog.

    python tools/exact_nuts_rates.py [--reps 5] [--out profiles/exact_nuts_rates.json]     # on the GPU

Every step is a child process of its own under a time limit (--cell NAME is what the child runs); the first step that fails ends the
run.  Every cell is reported, those where the new path loses included.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS, CS = (20, 64, 128), (1, 256, 2048)
TUNE, DRAWS, DEPTH = 50, 50, 8
HOST_TUNE, HOST_DRAWS = 30, 30
N_SETS = 64            # chain c samples data set c % N_SETS
STEP_LIMIT_S = 240


def data(N):
    import ggp_amd
    X, Y, _ = ggp_amd.identification_data(N, N_SETS, np.random.default_rng(57))
    return X, Y


def cell_nuts(N, C, reps):
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    X, Y = data(N)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    Xd, Yd = T(X), T(Y)
    rng = np.random.default_rng(N + C)
    q0 = np.array([np.log(2.0), 0.0, 0.0]) + rng.uniform(-0.5, 0.5, (C, 3))
    seeds = [int(s) for s in rng.integers(1, 2 ** 62, C)]
    iy = (np.arange(C) % N_SETS).astype(np.int32)

    def run(epl=None):
        return eng.exact_nuts_batch(Xd, Yd, q0, seeds, TUNE, DRAWS, iy=iy, max_treedepth=DEPTH, evals_per_launch=epl)

    def timed(epl=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = run(epl)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    run()  # warm-up: library, allocator, code object
    torch.cuda.synchronize()
    ms, r = [], None
    for _ in range(reps):
        t, r = timed()
        ms.append(t)
    med = statistics.median(ms)
    evals = int(r["evaluations"].sum())
    launches = int(r["launches"])
    row = {"N": N, "C": C, "reps": reps, "tune": TUNE, "draws": DRAWS, "run_ms": round(med, 3), "evaluations": evals,
           "leapfrogs_per_s": round(evals / (med * 1e-3), 1), "launches": launches, "ms_per_launch": round(med / launches, 3),
           "evals_per_launch": int(eng.exact_nuts_evals_per_launch(C, N)), "chains_per_cu": int(eng.exact_nuts_lib.sgp_exact_nuts_batch_occupancy(N, 0)),
           "bad_starts": int((r["info"] != 0).sum()), "diverging_share": float(r["stats"][:, :, 4].mean())}
    if C == 1:  # one chain, one launch: the latency of an evaluation (sampler step included) on one workgroup
        t1 = statistics.median([timed(1 << 30)[0] for _ in range(reps)])
        st = r["stats"][0]
        kept = float(st[-1, 7] - st[0, 7] + st[0, 1])  # evaluations of the kept draws: the cumulative count, less what preceded draw 0
        row.update(one_launch_ms=round(t1, 3), us_per_evaluation=round(1e3 * t1 / evals, 2),
                   device_clock_us_per_evaluation=round(1e6 * float(r["seconds"].sum()) / kept, 2))
    return row


def cell_host(N):
    import torch
    import ggp_amd
    eng = ggp_amd.HipEngine()
    X, Y = data(N)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=eng.device)  # noqa: E731
    tgt = ggp_amd.ExactHmcTarget(T(X), T(Y[0]), engine=eng)
    ggp_amd.sample_nuts(tgt, 3, 3, seed=1, max_treedepth=DEPTH)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr = ggp_amd.sample_nuts(tgt, HOST_DRAWS, HOST_TUNE, seed=2, max_treedepth=DEPTH)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"N": N, "tune": HOST_TUNE, "draws": HOST_DRAWS, "wall_s": round(wall, 4), "evaluations": int(tr.n_leapfrog),
            "leapfrogs_per_s": round(tr.n_leapfrog / wall, 1), "us_per_evaluation": round(1e6 * wall / tr.n_leapfrog, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/exact_nuts_rates.json")
    ap.add_argument("--cell", help="(internal) run one step in this process and print its JSON line")
    a = ap.parse_args()
    if a.cell:
        kind, *rest = a.cell.split(":")
        row = cell_host(int(rest[0])) if kind == "host" else cell_nuts(int(rest[0]), int(rest[1]), a.reps)
        print("RESULT " + json.dumps(row), flush=True)
        return
    rows, host = [], []
    for name in ["nuts:%d:%d" % (N, C) for N in NS for C in CS] + ["host:%d" % N for N in NS]:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--cell", name,
                            "--reps", str(a.reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-4000:])
            raise SystemExit("step %s ended with status %d: nothing more is started on the GPU" % (name, r.returncode))
        row = json.loads(line[0][len("RESULT "):])
        print(json.dumps(row), flush=True)
        (host if name.startswith("host") else rows).append(row)
    import torch
    base = {h["N"]: h["leapfrogs_per_s"] for h in host}
    for row in rows:
        row["over_host_driven"] = round(row["leapfrogs_per_s"] / base[row["N"]], 2)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "max_treedepth": DEPTH, "device_resident": rows,
                   "host_driven_sample_nuts": host}, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
