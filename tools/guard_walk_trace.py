#!/usr/bin/env python3
"""The guarded evaluation walk (core.py: CollapsedBound._evaluate) as a list of DISCRETE facts, on the CPU double: per evaluation the
engine methods called in order, the tier of every attempt, the tier accepted, `guard.open`, every counter and the trailing-word pause.
No floating-point value is recorded (another machine's BLAS may round differently); instead every number the walk compares against a
threshold -- each estimate against tol, tol / 2 and reach x tol, the guard's prediction likewise, the trailing word's correction against
`extended_lo_max_correction` -- is asserted to lie a factor 1.5 away from it, which makes the trace a property of the host logic alone.
tests/test_guard_walk_trace.py replays the walk against tests/golden/guard_walk_trace.json, recorded before the walk was rebuilt.
    python3 tools/guard_walk_trace.py [out.json]"""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARGIN = 1.5
# (lengthscale, s2): estimates from benign over the gradient ranges and the value range to beyond all of them
CELLS = [(0.8, 0.3), (3.0, 2e-2), (3.0, 5e-3), (5.0, 1.5e-3), (25.0, 1e-5), (2.0, 5e-2), (10.0, 1e-4), (1.2, 0.1), (2.0, 2e-7)]
LO_CELL = (3.0, 5e-3)   # between 3 x and 1000 x the tolerance: a gradient here rests on the trailing word
PASS1 = {"suffstats": 0, "suffstats_extended": 1, "suffstats_whitened": 2, "suffstats_whitened_rows": 2}
RECORDED = ("result_buffer", "kuu", "kuu_factor", "suffstats", "suffstats_extended", "suffstats_whitened", "suffstats_whitened_rows",
            "bound", "phibar_dd", "streaming_error_report", "suffstats_bwd", "suffstats_bwd_lo", "suffstats_bwd_factored", "kuu_bwd",
            "read_result", "read_estimate")
COUNTERS = ("n_evals", "n_grads", "n_collectives", "n_guard_reruns", "n_direct_whitened", "n_extended", "n_timeout_retries", "n_lo_rejections")


def _problem(N=600, M=24, d=3, seed=4):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X[:, 0]) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    return X, y, X[:M].clone()


def _recording(base):
    """`base` with every top-level call of a RECORDED method noted in `self.log` (what a method delegates to inside the double is not one)."""

    class Recording(base):
        def __init__(self, *a, **k):
            self.log, self.estimates, self._depth = [], [], 0
            super().__init__(*a, **k)

    def wrap(name):
        def method(self, *a, **k):
            if self._depth == 0:
                self.log.append(name)
            self._depth += 1
            try:
                r = getattr(super(Recording, self), name)(*a, **k)
            finally:
                self._depth -= 1
            if name == "read_estimate":
                self.estimates.append(r)
            return r
        return method

    for name in RECORDED:
        setattr(Recording, name, wrap(name))
    return Recording


def _engines():
    from fake_engine import FactoredOracleEngine

    class BrokenB(FactoredOracleEngine):   # the streaming order "fails" at small noise: B not positive definite
        def bound(self, Kuu, packed, s2, N, with_adjoints=False, want_factors=False, result=None, kuu_linv=None, whitened=False, want_cw=False):
            res = super().bound(Kuu, packed, s2, N, with_adjoints, want_factors, result, kuu_linv, whitened, want_cw)
            if not whitened and float(s2) < 1e-3:
                res["info"][0] = Kuu.shape[0] + 5
                res["out"].fill_(float("nan"))
            return res

    class Starved(FactoredOracleEngine):   # the status word a starved single-launch Cholesky leaves, until the shared-device mode is on
        OPTIONS = {"shared_device": 6}

        def __init__(self, heals):
            super().__init__()
            self.opt, self.heals = {"shared_device": 0.0}, heals

        def set_option(self, name, value):
            prev, self.opt[name] = self.opt[name], float(value)
            return prev

        def get_option(self, name):
            return self.opt[name]

        def bound(self, *a, **k):
            res = super().bound(*a, **k)
            if self.opt["shared_device"] == 0.0 or not self.heals:
                res["info"][0] = -7777
            return res

    return _recording(FactoredOracleEngine), _recording(BrokenB), _recording(Starved)


def _apart(x, threshold, what):
    if math.isfinite(x) and x > 0.0:
        assert x * MARGIN <= threshold or x >= MARGIN * threshold, "%s: %.3e is within %.1f x of the threshold %.3e" % (what, x, MARGIN, threshold)


class _Walk:
    def __init__(self, trace, mode, bound, Z):
        self.trace, self.mode, self.cb, self.Z = trace, mode, bound, Z

    def step(self, cell, call="value", **kw):
        cb, eng = self.cb, self.cb.engine
        ls, s2 = cell
        with_grad = call == "value_and_grad"
        reach = cb.extended_range
        if with_grad:
            reach = kw.get("grad_reach") or (cb.extended_grad_range_lo if cb._bwd_lo_ok(self.Z.shape[0]) else cb.extended_grad_range)
        tol = cb.streaming_tol
        what = "%s %s %s" % (self.mode, call, cell)
        if cb.guard.open:
            _apart(cb.guard.predicted, reach * tol, what + " (start: prediction)")
        del eng.log[:], eng.estimates[:]
        lo_before, raised = cb.last_lo_correction, None
        try:
            if call == "factors":
                cb.factors(self.Z, [ls] * 3, 1.0, s2)
            else:
                getattr(cb, call)(self.Z, [ls] * 3, 1.0, s2, **kw)
        except Exception as exc:   # (the kind is a discrete fact as well)
            raised = type(exc).__name__
        for est in eng.estimates:
            for thr in (tol, 0.5 * tol, reach * tol):
                _apart(est, thr, what + " (estimate)")
        for thr in (tol, 0.5 * tol):
            _apart(cb.guard.predicted, thr, what + " (prediction)")
        if cb.last_lo_correction is not lo_before and cb.last_lo_correction is not None:
            _apart(cb.last_lo_correction, cb.extended_lo_max_correction, what + " (correction)")
        self.trace.append({"mode": self.mode, "call": call, "cell": list(cell), "calls": " ".join(eng.log),
                           "tiers": [PASS1[n] for n in eng.log if n in PASS1], "accepted": cb.last_tier, "open": bool(cb.guard.open),
                           "counters": [getattr(cb, n) for n in COUNTERS], "lo_skip": cb._lo_skip, "lo_pause": cb._lo_pause, "raised": raised})


def record():
    """The trace: a list of dicts, one per evaluation."""
    import ggp_amd as pkg
    Plain, BrokenB, Starved = _engines()
    X, y, Z = _problem()
    trace = []
    old = pkg.CollapsedBound.WHITENED_MAX_WORK
    pkg.CollapsedBound.WHITENED_MAX_WORK = 0   # form="auto" would take the whitened order for problems this small
    try:
        def walk(mode, engine=None, **attrs):
            cb = pkg.CollapsedBound(X, y, jitter=1e-6, engine=engine or Plain())
            cb.whitened_rows_min_work = 0
            for k, v in attrs.items():
                setattr(cb, k, v)
            return _Walk(trace, mode, cb, Z)

        sampler = {"grad_reach": 16384.0, "strict": True}
        for mode, call, kw, attrs in (("value", "value", {}, {}), ("value_strict", "value", {"strict": True}, {}),
                                      ("grad", "value_and_grad", {"raise_on_fail": False}, {}),
                                      ("grad_strict", "value_and_grad", {"raise_on_fail": False, "strict": True}, {}),
                                      ("sampler", "value_and_grad", dict(sampler, raise_on_fail=False), {}),
                                      ("grad_status_first", "value_and_grad", {"raise_on_fail": False}, {"early_check_min_work": 0}),
                                      ("sampler_status_first", "value_and_grad", dict(sampler, raise_on_fail=False), {"early_check_min_work": 0}),
                                      ("grad_gz", "value_and_grad", {"raise_on_fail": False, "want_gz": True}, {}),
                                      ("factors", "factors", {}, {})):
            w = walk(mode, **attrs)
            for cell in CELLS:
                w.step(cell, call, **kw)
        # strict evaluations on a memory that under-predicts / over-predicts: down at most once, up always
        for ratio, predicted in ((1e-12, 0.0), (1.0, 1.0)):
            for cell in ((25.0, 1e-5), (0.8, 0.3), (2.0, 2e-7)):
                w = walk("memory_%g_%g" % (ratio, predicted))
                w.cb.guard.open, w.cb.guard.ratio, w.cb.guard.predicted = True, ratio, predicted
                w.step(cell, "value_and_grad", **dict(sampler, raise_on_fail=False))
                w.step(cell, "value", strict=True)
        # a trailing-word rejection through its pause (8), the second rejection (16) and the recovery
        w = walk("lo_rejection")
        w.cb.engine.lo_delta_scale = 1e12
        for _ in range(9):
            w.step(LO_CELL, "value_and_grad")
        w.step(LO_CELL, "value")
        w.step(LO_CELL, "value_and_grad")
        w.step(LO_CELL, "value_and_grad", **sampler)       # the sampler mode takes the gradient whatever the correction says
        w.cb.engine.lo_delta_scale = 1.0
        for _ in range(17):
            w.step(LO_CELL, "value_and_grad")
        w = walk("lo_nan")
        w.cb.engine.lo_delta_scale = float("nan")
        w.step(LO_CELL, "value_and_grad")
        w.step(CELLS[0], "value_and_grad")
        # a failed factorization of B below the whitened order is a guard trip; one of K_uu is the matrix's, whatever the tier
        w = walk("b_failure", BrokenB())
        for cell in ((25.0, 1e-5), (0.8, 0.3), (10.0, 1e-4)):
            w.step(cell, "value")
            w.step(cell, "value_and_grad")
        w = walk("kuu_failure", jitter=0.0)
        w.Z = Z.clone()
        w.Z[1] = w.Z[0]
        w.step(CELLS[0], "value", raise_on_fail=False)
        w.step(CELLS[0], "value")
        w.step(CELLS[0], "value_and_grad", raise_on_fail=False)
        # a device time-out: healed by the shared-device mode, and not
        for heals in (True, False):
            w = walk("timeout_%s" % ("healed" if heals else "unhealed"), Starved(heals))
            w.step(CELLS[0], "value")
            w.step(CELLS[0], "value_and_grad")
    finally:
        pkg.CollapsedBound.WHITENED_MAX_WORK = old
    return trace


COLUMNS = ("mode", "call", "cell", "calls", "tiers", "accepted", "open", "counters", "lo_skip", "lo_pause", "raised")


def dumps(trace):
    """The file: every distinct call sequence once, then one row per evaluation (COLUMNS; `calls` is the sequence's index)."""
    seqs = []
    for t in trace:
        if t["calls"] not in seqs:
            seqs.append(t["calls"])
    rows = [json.dumps([seqs.index(t[c]) if c == "calls" else t[c] for c in COLUMNS], separators=(",", ":")) for t in trace]
    return ('{"columns":' + json.dumps(COLUMNS) + ',"counters":' + json.dumps(COUNTERS) + ',"sequences":[\n' + ",\n".join(json.dumps(q) for q in seqs)
            + '\n],"evaluations":[\n' + ",\n".join(rows) + "\n]}\n")


def loads(text):
    doc = json.loads(text)
    rows = [dict(zip(doc["columns"], r)) for r in doc["evaluations"]]
    return [dict(t, calls=doc["sequences"][t["calls"]]) for t in rows]


if __name__ == "__main__":
    text = dumps(record())
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
