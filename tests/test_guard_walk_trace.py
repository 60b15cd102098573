"""The guarded evaluation walk, replayed against the trace recorded before `CollapsedBound._evaluate` was rebuilt around one typed attempt
(tools/guard_walk_trace.py; tests/golden/guard_walk_trace.json): per evaluation the engine calls in order, the tier of every attempt, the
accepted tier, `guard.open`, every counter and the trailing-word pause -- equal entry for entry.  The trace holds discrete facts only, and
the recorder asserts that every number the walk compares against a threshold lies a factor 1.5 away from it, so it does not depend on the
BLAS of the machine.  The reference has no counterpart of the guard (its op order is the whitened one: models/bayesian_sgpr_hmc.py:66,71)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _recorder():
    spec = importlib.util.spec_from_file_location("guard_walk_trace", os.path.join(ROOT, "tools", "guard_walk_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_walk_replays_the_recorded_trace_entry_for_entry():
    rec = _recorder()
    with open(os.path.join(ROOT, "tests", "golden", "guard_walk_trace.json")) as f:
        want = rec.loads(f.read())
    got = rec.loads(rec.dumps(rec.record()))   # (through the file's own form: tuples and lists compare alike)
    modes = {t["mode"] for t in want}
    assert {"value", "grad", "grad_strict", "sampler", "lo_rejection", "lo_nan", "b_failure", "kuu_failure", "timeout_healed",
            "timeout_unhealed"} <= modes
    for k, (w, g) in enumerate(zip(want, got)):
        assert g == w, (k, w["mode"], w["call"], w["cell"], {c: (w[c], g[c]) for c in w if w[c] != g[c]})
    assert len(got) == len(want)
