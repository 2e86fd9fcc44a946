"""`--clip` (Food-101 on stored CLIP features, CLIPClassifier) on one MI355X: time of the MLA step (two head-only phases) with the
fused phase (mla_feature_phase: 4 launches per projecting phase) and with MLA_FEATURE_FUSED=0 semantics (the general chain: 7
launches and a copy), batches served by CLIPFeatureBatcher from a synthetic feature directory.  The two trainers alternate in one
process: warm-up, then three timed windows each of at least a second of steps, every window ended by a device synchronise; the
figure is the median window, the spread its min .. max.  Also the phase alone (device events around back-to-back calls).
--gs-mode as_intended,owm adds the same two trainers with the scalar-denominator projector (mla_feature_phase_owm: 3 launches per
projecting phase) to the alternation, as "fused_owm" and "chain_owm".  Not the headline bench line; numbers go to DESIGN.md
section 15 and the README."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mla_hip import CLIPClassifier, CLIPFeatureBatcher, MLATrainer  # noqa: E402

B, D, C = int(os.environ.get("B", "64")), int(os.environ.get("D", "512")), int(os.environ.get("C", "101"))
N = int(os.environ.get("N", "2048"))
WINDOW_S, REPEATS = float(os.environ.get("WINDOW_S", "1.0")), 3
ap = argparse.ArgumentParser()
ap.add_argument("--gs-mode", default="as_intended", help="comma-separated GSPlugin modes to time: as_intended, owm")
GS_MODES = ap.parse_args().gs_mode.split(",")
assert torch.cuda.is_available(), "bench_clip.py measures on the GPU"


class Args:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


def feature_dir(root):
    rng = np.random.default_rng(0)
    names = [f"s{i:05d}" for i in range(N)]
    for sub in ("text", "visual"):
        os.makedirs(os.path.join(root, sub))
        for n in names:
            np.save(os.path.join(root, sub, n + ".npy"), np.abs(rng.standard_normal((1, D)) * 0.7 + 0.3).astype(np.float32))
    return names, [int(v) for v in rng.integers(0, C, N)]


def epoch(tr, bt, e):
    bt.set_epoch(e)
    for step, (tok, img, label, _idx) in enumerate(bt):
        tr.train_step(tok, img, label, step, len(bt))
    return len(bt)


with tempfile.TemporaryDirectory() as root:
    names, labels = feature_dir(root)
    bt = CLIPFeatureBatcher(names, labels, B, os.path.join(root, "text"), os.path.join(root, "visual"), shuffle=True, seed=0, drop_last=True)
trainers = {}
for mode in GS_MODES:
    for name, fused in (("fused", True), ("chain", False)):
        tr = MLATrainer(CLIPClassifier(Args(), seed=1, feat_dim=D), lr=1e-3, gs_mode=mode)
        tr.fused_feature_phase = fused
        trainers[name if mode == "as_intended" else f"{name}_{mode}"] = tr
for tr in trainers.values():                                 # warm-up: code objects, buffers, the projection firing
    epoch(tr, bt, 0)
torch.cuda.synchronize()
windows = {k: [] for k in trainers}
e = 1
for _rep in range(REPEATS):
    for name, tr in trainers.items():                        # alternate them in one process
        steps, t0 = 0, time.perf_counter()
        while True:
            steps += epoch(tr, bt, e)
            e += 1
            torch.cuda.synchronize()                         # the window ends on finished work
            dt = time.perf_counter() - t0
            if dt >= WINDOW_S:
                break
        windows[name].append(dt / steps * 1e6)
result = {"batch": B, "D": D, "C": C, "window_s": WINDOW_S, "gs_modes": GS_MODES}
for name, w in windows.items():
    w = sorted(w)
    result[name] = {"us_per_step": w[1], "min": w[0], "max": w[2]}
    print(f"CLIP MLA step ({name}): B={B} D={D} C={C}: {w[1]:.1f} us/step (min {w[0]:.1f}, max {w[2]:.1f} over {REPEATS} windows), "
          f"{B / w[1] * 1e6:.0f} samples/s")
# ---- the projecting phase alone, on the device clock: back-to-back calls on one stream
tok, img, label, _ = next(iter(bt))
for name, tr in trainers.items():
    reps = 200
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(10):
        tr.train_step(tok, img, label, 1, 10)
    ev[0].record()
    for _ in range(reps):
        tr.train_step(tok, img, label, 1, 10)
    ev[1].record()
    torch.cuda.synchronize()
    us = ev[0].elapsed_time(ev[1]) * 1e3 / (2 * reps)
    result[name]["us_per_phase_device"] = us
    print(f"CLIP phase ({name}): {us:.1f} us per projecting phase (device events, {2 * reps} phases back to back)")
print(json.dumps(result))
