"""The CREMA-D batch-64 MLA step under each conv arithmetic, same process, same box: f32 (exact fp32 MFMA), split (six bf16
products, fp32-equivalent, the shipped default) and bf16 (operands rounded once, one product).  Shapes of CREMA-D config 1
(per-GPU batch 64, spectrogram 1x1024x128, frames 3x3x224x224, 6 classes).  One JSON line per arithmetic with ms/step and
samples/s, each with its ratio to the split step of this run.  Not the headline bench line (bench.py); numbers go to DESIGN.md 4a.

    python scripts/bench_math.py [--steps 20] [--warmup 5] [--batch 64] [--maths f32,split,bf16] [--serial]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch  # noqa: E402

from mla_hip import AVClassifier, MLATrainer  # noqa: E402

SPEC_HW, FRAMES, IMG_HW = (1024, 128), 3, (224, 224)
MATHS = ("f32", "split", "bf16")


def timed(step, steps, warmup):
    for s in range(warmup):
        step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        step(warmup + s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


class MLAArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--maths", default=",".join(MATHS), help="comma-separated subset, in run order (e.g. one arithmetic per profiler run)")
    ap.add_argument("--serial", action="store_true", help="set_overlap(False): no per-encoder stream pipeline, kernels serialized")
    a = ap.parse_args()
    maths = a.maths.split(",")
    if not set(maths) <= set(MATHS):
        ap.error(f"--maths: choose from {MATHS}")
    B = a.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    spec = torch.randn((B,) + SPEC_HW, device="cuda", generator=g) * 4.4849 - 5.081
    image = torch.randn((B, 3, FRAMES) + IMG_HW, device="cuda", generator=g)
    label = torch.randint(0, 6, (B,), device="cuda", generator=g)
    rows = []
    for math in maths:
        model = AVClassifier(MLAArgs(), seed=1, conv_math=math)
        tr = MLATrainer(model)
        if a.serial:
            tr.set_overlap(False)
        dt = timed(lambda s: tr.train_step(spec, image, label, s % 100, 100), a.steps, a.warmup)
        tr.join()
        rows.append({"mode": "MLA", "conv_math": math, "batch": B, "steps": a.steps, "warmup": a.warmup, "serial": a.serial,
                     "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 1)})
        del tr, model
        torch.cuda.empty_cache()
    split_ms = next((r["ms_per_step"] for r in rows if r["conv_math"] == "split"), None)
    for r in rows:
        if split_ms:
            r["vs_split"] = round(r["ms_per_step"] / split_ms, 4)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
