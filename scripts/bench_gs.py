"""The head-gradient projection alone on one MI355X: mla_gs_project (the literal utils/utils.py:34-41: three launches and a
device-to-device copy) against mla_gs_project_owm (gs_mode="owm": two launches, no copy, one pass over Pl fewer) at the head shapes
(D, C) = (512, 6) and (768, 101).  The two alternate in one process on one stream: warm-up, then three timed windows each of at
least half a second of back-to-back calls, every window ended by a device synchronise; the figure is the median window, the spread
its min .. max.  Pl is reset to the identity before every window (the literal rule's Pl collapses when it runs free).  Not the
headline bench line; numbers go to DESIGN.md sections 9 / 15 and the README."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch  # noqa: E402
from mla_hip import ops  # noqa: E402

SHAPES = [(512, 6), (768, 101)]
WINDOW_S, REPEATS, CHUNK = float(os.environ.get("WINDOW_S", "0.5")), 3, 200
assert torch.cuda.is_available(), "bench_gs.py measures on the GPU"

result = {"window_s": WINDOW_S}
for D, C in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(D + C)
    r = torch.randn(D, device="cuda", generator=g) * 0.7 + 0.3            # a feature mean of both signs
    G0 = torch.randn(C, D, device="cuda", generator=g)
    Pl, G = torch.eye(D, device="cuda"), G0.clone()
    rules = {"literal": (ops.gs_project, torch.empty(ops.gs_ws_elems(D, C), device="cuda")),
             "owm": (ops.gs_project_owm, torch.empty(ops.gs_owm_ws_elems(D, C), device="cuda"))}
    for fn, ws in rules.values():                                          # warm-up: code objects
        for _ in range(20):
            fn(Pl, r, G, 0.1, ws)
    torch.cuda.synchronize()
    windows = {k: [] for k in rules}
    for _rep in range(REPEATS):
        for name, (fn, ws) in rules.items():                               # alternate the two in one process
            Pl.copy_(torch.eye(D, device="cuda"))
            G.copy_(G0)
            torch.cuda.synchronize()
            calls, t0 = 0, time.perf_counter()
            while True:
                for _ in range(CHUNK):
                    fn(Pl, r, G, 0.1, ws)
                calls += CHUNK
                torch.cuda.synchronize()                                   # the window ends on finished work
                dt = time.perf_counter() - t0
                if dt >= WINDOW_S:
                    break
            windows[name].append(dt / calls * 1e6)
    key = f"D{D}_C{C}"
    result[key] = {}
    for name, w in windows.items():
        w = sorted(w)
        result[key][name] = {"us_per_call": w[1], "min": w[0], "max": w[2]}
        print(f"GS projection ({name}): D={D} C={C}: {w[1]:.1f} us/call (min {w[0]:.1f}, max {w[2]:.1f} over {REPEATS} windows)")
print(json.dumps(result))
