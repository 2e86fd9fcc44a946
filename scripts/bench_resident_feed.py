"""The HBM-resident CREMA-D feed on one MI355X (numbers go to DESIGN.md section 9 and the README; no pass/fail threshold).

    python scripts/bench_resident_feed.py [--batch 64] [--steps 12] [--runs 3] [--frame 360x480]

Synthetic JPEGs and fbank .npy files as scripts/bench_frames.py writes them; `--samples` distinct clips are repeated to fill the
epoch (the store uploads every repetition, as it would distinct clips).  One process, one session, so the rates are comparable; the
step sources are measured in turn, `--runs` rounds of all of them.  One JSON line per item:
  build      ResidentStore from the decode_frames cache: seconds and resident bytes, also per 1 000 clips
  launches   (a) the three launches of a batch (draw, resample, gather) on the device clock, HIP events, warm
  step       MLATrainer samples/s fed from
               (b) device_tensors   tensors already on the device: bench.py's input
               (c) cache            FrameBatcher(frame_cache, threads=1) + DeviceFeeder
               (d) resident         ResidentFrameBatcher (train, shuffle)
             every run, and per source the median with the spread (max - min) / median
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_frames import emit, make_trainer, timed_epoch, write_dataset  # noqa: E402
from mla_hip import DeviceFeeder, FrameBatcher, ResidentFrameBatcher, ResidentStore, decode_frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--frame", default="360x480")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resident_feed needs a GPU"
    H, W = (int(v) for v in a.frame.split("x"))
    B, T = a.batch, 3
    with tempfile.TemporaryDirectory() as tmp:
        base, audio, visual = write_dataset(tmp, a.samples, H, W)
        cache = os.path.join(tmp, "cache")
        decode_frames(visual, cache, base)
        names = (base * ((B * a.steps + len(base) - 1) // len(base)))[:B * a.steps]
        labels = [i % 6 for i in range(len(names))]

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = ResidentStore(names, labels, frame_cache=cache, audio_feature_path=audio)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        emit(item="build", clips=len(names), frame=f"{H}x{W}", seconds=round(dt, 3), resident_mb=round(store.nbytes / 1e6, 1),
             seconds_per_1000_clips=round(dt * 1000 / len(names), 2), resident_mb_per_1000_clips=round(store.nbytes * 1000 / len(names) / 1e6, 1))

        rb = ResidentFrameBatcher(names, labels, B, store=store, train=True, shuffle=True, seed=1)
        per_run = []
        for r in range(a.runs):
            rb.set_epoch(r)
            for _ in rb:                                         # warm: every slot exists, the kernels are loaded
                pass
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            n = sum(1 for _ in rb)
            ev[1].record()
            torch.cuda.synchronize()
            per_run.append(ev[0].elapsed_time(ev[1]) / n)
        med = statistics.median(per_run)
        emit(item="launches", batch=B, frame=f"{H}x{W}", ms_per_batch=[round(v, 4) for v in per_run], median_ms=round(med, 4),
             spread=round((max(per_run) - min(per_run)) / med, 4))

        tr = make_trainer()
        g = torch.Generator(device="cuda").manual_seed(0)
        spec = torch.randn((B, 1024, 128), device="cuda", generator=g)
        image = torch.randn((B, 3, T, 224, 224), device="cuda", generator=g)
        label = torch.randint(0, 6, (B,), device="cuda", generator=g)
        rates = {"device_tensors": [], "cache": [], "resident": []}
        for r in range(a.runs):
            rates["device_tensors"].append(timed_epoch(tr, [(spec, image, label)] * a.steps, a.warm))
            fb = FrameBatcher(names, labels, B, audio, frame_cache=cache, threads=1, pin=True, epoch=r)
            rates["cache"].append(timed_epoch(tr, DeviceFeeder(fb, depth=3), a.warm))
            fb.close()
            rb.set_epoch(r)
            rates["resident"].append(timed_epoch(tr, rb, a.warm))
        for source, v in rates.items():
            med = statistics.median(v)
            emit(item="step", source=source, batch=B, samples_per_s=[round(x, 1) for x in v], median=round(med, 1),
                 spread=round((max(v) - min(v)) / med, 4))


if __name__ == "__main__":
    main()
