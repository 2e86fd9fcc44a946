"""Joint concat-fusion step (gs_flag false, main.py:164-417) vs the MLA step, same process, same box: CREMA-D config 1
shapes (per-GPU batch 64, spectrogram 1x1024x128, frames 3x3x224x224, 6 classes), conv arithmetic split (the shipped
default) unless MATH=f32.  One JSON line per mode (MLA, Normal, OGM, OGM_GE; QMF on request) with samples/s and ms/step.  Not the headline
bench line (bench.py); numbers go to DESIGN.md.

    python scripts/bench_joint.py [--steps 20] [--warmup 5] [--batch 64] [--math split] [--serial]
    python scripts/bench_joint.py --fusion concat,sum,film,gated      # the joint Normal step per fusion head (mla_hip.attach_fusion)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
import torch  # noqa: E402

from mla_hip import AVClassifier, JointTrainer, MLATrainer, QMFTrainer, attach_fusion  # noqa: E402

SPEC_HW, FRAMES, IMG_HW = (1024, 128), 3, (224, 224)


def timed(step, steps, warmup):
    for s in range(warmup):
        step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        step(warmup + s)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--math", choices=["f32", "split"], default=os.environ.get("MLA_CONV_MATH", "split"))
    ap.add_argument("--modes", default="MLA,Normal,OGM,OGM_GE", help="comma-separated subset (e.g. one mode per profiler run); QMF is also a mode")
    ap.add_argument("--serial", action="store_true", help="joint modes with set_overlap(False) (A/B of the concurrent backwards)")
    ap.add_argument("--fusion", default="", help="comma-separated subset of concat,sum,film,gated: instead of the modes, time the joint "
                    "Normal step per fusion in ONE process, alternating, three runs each; one JSON line per fusion with the median ms/step "
                    "and (max - min) / median")
    a = ap.parse_args()
    B = a.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    spec = torch.randn((B,) + SPEC_HW, device="cuda", generator=g) * 4.4849 - 5.081
    image = torch.randn((B, 3, FRAMES) + IMG_HW, device="cuda", generator=g)
    label = torch.randint(0, 6, (B,), device="cuda", generator=g)
    base = {"batch": B, "conv_math": a.math, "steps": a.steps, "warmup": a.warmup}

    if a.fusion:
        fusions = a.fusion.split(",")
        trainers = {}
        for f in fusions:
            class FArgs:
                fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
            model = AVClassifier(FArgs(), seed=1, conv_math=a.math)
            if f != "concat":
                attach_fusion(model, f, seed=2)
            trainers[f] = JointTrainer(model)
            if a.serial:
                trainers[f].set_overlap(False)
        runs = {f: [] for f in fusions}
        for _ in range(3):                                            # alternating: drift of the box hits every fusion alike
            for f in fusions:
                jt = trainers[f]
                runs[f].append(timed(lambda s: jt.train_step(spec, image, label, s), a.steps, a.warmup) * 1e3)
        for f in fusions:
            ms = sorted(runs[f])
            print(json.dumps(dict(base, fusion=f, ms_per_step=round(ms[1], 3), runs_ms=[round(v, 3) for v in runs[f]],
                                  spread=round((ms[2] - ms[0]) / ms[1], 4), samples_per_s=round(B / ms[1] * 1e3, 1),
                                  loss=round(trainers[f].losses["loss"].item(), 5))), flush=True)
        return
    modes = a.modes.split(",")
    mla_ms = None
    if "MLA" in modes:
        class MLAArgs:
            fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"
        model = AVClassifier(MLAArgs(), seed=1, conv_math=a.math)
        tr = MLATrainer(model)
        dt = timed(lambda s: tr.train_step(spec, image, label, s % 100, 100), a.steps, a.warmup)
        print(json.dumps(dict(base, mode="MLA", ms_per_step=round(dt * 1e3, 3), samples_per_s=round(B / dt, 1))), flush=True)
        mla_ms = dt * 1e3
        del tr, model
    for mode in [m for m in ("Normal", "OGM", "OGM_GE") if m in modes]:
        class Args:
            fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, mode
        model = AVClassifier(Args(), seed=1, conv_math=a.math)
        jt = JointTrainer(model, modulation=mode, alpha=0.3, modulation_starts=0, modulation_ends=10 ** 9)
        if a.serial:
            jt.set_overlap(False)
        dt = timed(lambda s: jt.train_step(spec, image, label, s), a.steps, a.warmup)
        print(json.dumps(dict(base, mode=mode, overlap=jt.overlap_forward, ms_per_step=round(dt * 1e3, 3), samples_per_s=round(B / dt, 1),
                              vs_mla_ms=None if mla_ms is None else round(dt * 1e3 - mla_ms, 3), loss=round(jt.losses["loss"].item(), 5))), flush=True)
        del jt, model
    if "QMF" in modes:
        class QArgs:
            fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
        n_data = 6698                                             # CREMA-D training split
        model = AVClassifier(QArgs(), seed=1, conv_math=a.math)
        qt = QMFTrainer(model, n_data, seed=2)
        if a.serial:
            qt.set_overlap(False)
        idx = torch.randperm(n_data, device="cuda", generator=g)[:B]
        dt = timed(lambda s: qt.train_step(spec, image, label, (idx + s * B) % n_data, s), a.steps, a.warmup)
        print(json.dumps(dict(base, mode="QMF", overlap=qt.overlap_forward, ms_per_step=round(dt * 1e3, 3), samples_per_s=round(B / dt, 1),
                              vs_mla_ms=None if mla_ms is None else round(dt * 1e3 - mla_ms, 3), loss=round(qt.losses["loss"].item(), 5))), flush=True)
        del qt, model


if __name__ == "__main__":
    main()
