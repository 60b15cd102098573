"""Exact-GP (GPR_HMC) rates: ms per value and per value + gradient of sgp_exact_eval (HIP events, warm-up, median of repeats) at the
UCI sets' N and d, an A/B in the same process of the fused gradient (exact_grad_kernel) against a composition of existing pieces
(A^-1 = L^-T L^-1 formed explicitly by a GEMM, then sgp_kuu_bwd with Kuubar = G / 2 -- in this tool only, not in the library), and
the wall-clock of GPR_HMC.train_model() (50 tune + 10 draws) at the five UCI shapes.

    python tools/gpr_hmc_rates.py [--reps 20] [--train] [--out profiles/gpr_hmc_rates.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggp_amd  # noqa: E402

# (name, N_train, d): the reference's datasets at prop = 0.9 (Yacht, Boston, Energy, Concrete, WineRed), then two larger N
SHAPES = [("yacht", 277, 6), ("boston", 455, 13), ("energy", 691, 8), ("concrete", 927, 8), ("winered", 1439, 11),
          ("n2048", 2048, 8), ("n4096", 4096, 8)]


def problem(N, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    y = np.sin(2.0 * X @ w) + 0.3 * X[:, 0] + 0.1 * rng.standard_normal(N)
    return (X - X.mean(0)) / X.std(0), (y - y.mean()) / y.std()


def timed(fn, reps, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="also time GPR_HMC.train_model() at the five UCI shapes")
    ap.add_argument("--out", default="profiles/gpr_hmc_rates.json")
    a = ap.parse_args()
    eng = ggp_amd.HipEngine()
    lib = eng.lib
    rows = []
    for name, N, d in SHAPES:
        X, y = problem(N, d)
        Xd = torch.as_tensor(X, dtype=torch.float64, device=eng.device).contiguous()
        yd = torch.as_tensor(y, dtype=torch.float64, device=eng.device).contiguous()
        ls, sf2, s2 = [1.5] * d, 1.0, 0.1
        Np = int(math.sqrt(lib.sgp_exact_factors_len(N) + 0.25) - 0.5)  # len = Np^2 + Np
        H = eng.EXACT_HEAD
        buf = eng.empty(H + d + 2)
        info = buf[4:5].view(torch.int32)[:1]
        fac = eng.empty(lib.sgp_exact_factors_len(N))
        ws = eng._workspace("exact", lib.sgp_exact_workspace_bytes(N, d, 1))
        import ctypes as C

        def call(with_grad):  # the entry point alone (no host copy): what the device spends per evaluation
            st = lib.sgp_ctx_exact_eval(eng._c(), eng._ptr(Xd), d, eng._ptr(yd), N, d, eng._inv_ls(ls, d), sf2, s2, 0, with_grad,
                                        C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 8 * H), eng._ptr(fac), eng._ptr(info),
                                        eng._ptr(ws), ws.numel(), eng._stream())
            assert st == 0

        v_ms = timed(lambda: call(0), a.reps)
        vg_ms = timed(lambda: call(1), a.reps)
        r = eng.exact_eval(Xd, yd, ls, sf2, s2, want_factors=True)
        assert r["info"] == 0, r["info"]
        Linv = r["factors"][:Np * Np].view(Np, Np)[:N, :N]
        alpha = r["factors"][Np * Np:Np * Np + N]
        grads = eng.empty(d + 2)

        def composed():  # A^-1 by GEMM, G / 2, sgp_kuu_bwd (totals only)
            Ainv = Linv.T @ Linv
            Kb = 0.5 * (torch.outer(alpha, alpha) - Ainv)
            grads.zero_()
            eng.kuu_bwd(Xd, ls, sf2, Kb.contiguous(), grads)

        comp_ms = timed(composed, a.reps)
        composed()
        torch.cuda.synchronize()
        g_comp = grads.cpu().tolist()[:d + 1]
        g_fused = r["ls"] + [r["sf2"]]
        rel = max(abs(p - q) for p, q in zip(g_comp, g_fused)) / max(1.0, max(abs(q) for q in g_fused))
        rows.append({"shape": name, "N": N, "d": d, "ms_value": round(v_ms, 4), "ms_value_grad": round(vg_ms, 4),
                     "ms_fused_gradient": round(vg_ms - v_ms, 4), "ms_composed_gradient": round(comp_ms, 4),
                     "composed_vs_fused_max_rel_diff": rel,
                     "grad_tflops_n3_over_3": round((N ** 3 / 3.0) / ((vg_ms - v_ms) * 1e-3) / 1e12, 3) if vg_ms > v_ms else None})
        print(json.dumps(rows[-1]), flush=True)
    train = []
    if a.train:
        for name, N, d in SHAPES[:5]:
            X, y = problem(N, d, 1)
            m = ggp_amd.GPR_HMC(torch.as_tensor(X, device=eng.device), torch.as_tensor(y, device=eng.device), ggp_amd.GaussianLikelihood(),
                                engine=eng, seed=0)
            t0 = time.perf_counter()
            tr, step, perf = m.train_model()
            wall = time.perf_counter() - t0
            train.append({"shape": name, "N": N, "d": d, "train_model_s": round(wall, 3), "sampler_perf_s": round(float(perf[0]), 3),
                          "leapfrog_evals": m._exact_target().n_evals, "step_size": float(step[0])})
            print(json.dumps(train[-1]), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rates": rows, "train_model": train,
           "reference_gpr_hmc_s": {"boston": 27.88, "concrete": 252.16, "energy": 89.92, "winered": 478.54, "yacht": 10.19}}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
