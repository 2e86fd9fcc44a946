"""How bench_eval.py, bench_metrics.py and bench_sweep.py time: the forms alternate in one process, warm-up, then REPEATS windows each,
every window at least WINDOW_S of back-to-back calls on one stream ended by a device synchronise (host clock: launch overhead is part
of what these scripts compare).  The figure is the median window, the spread (max - min) / median."""
import os
import time

import torch

WINDOW_S, REPEATS = float(os.environ.get("WINDOW_S", "0.5")), 3


def windows(forms, warmup=None):
    """forms: name -> (callable running one unit of work, units per call[, calls between two looks at the clock: 1 for a call that
    takes milliseconds and ends in a host sync of its own; default 50 units' worth]).  warmup: calls of each form before the first
    window (default 20 units' worth, at most one look's).  -> name -> sorted us per unit of the REPEATS windows."""
    forms = {k: (v[0], v[1], v[2] if len(v) > 2 else max(1, 50 // v[1])) for k, v in forms.items()}
    for fn, units, inner in forms.values():                  # warm-up: code objects, buffers
        for _ in range(min(inner, max(1, 20 // units)) if warmup is None else warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _rep in range(REPEATS):
        for name, (fn, units, inner) in forms.items():       # alternate the forms in one process
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(inner):
                    fn()
                n += inner * units
                torch.cuda.synchronize()                     # the window ends on finished work
                dt = time.perf_counter() - t0
                if dt >= WINDOW_S:
                    break
            out[name].append(dt / n * 1e6)
    return {k: sorted(v) for k, v in out.items()}


def summary(w):
    return {"us": w[1], "min": w[0], "max": w[2], "spread": (w[2] - w[0]) / w[1]}


def verdict(base, new, both=False, what="the spread"):
    """`new` against `base`, judged by base's own spread, or with both=True by the larger of the two spreads."""
    gap, spread = (new["us"] - base["us"]) / base["us"], max(base["spread"], new["spread"] if both else 0.0)
    if abs(gap) <= spread:
        return f"inside {what} ({gap:+.1%} vs {spread:.1%})"
    return f"{'slower' if gap > 0 else 'faster'} beyond {what} ({gap:+.1%} vs {spread:.1%})"
