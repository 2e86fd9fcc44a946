"""M3AE batch feed: kernel times, host feed rates and the MLA step fed from the batcher (one JSON line per item).

    python scripts/bench_m3ae_feed.py [--batch 64] [--steps 8] [--frame 384x512] [--depth 12] [--runs 7]

Synthetic JPEGs (smooth gradients + noise, PIL quality 90, a Food-101-sized image) and token / padding-mask .npy files are
written to a temporary directory; `--samples` distinct images are repeated to fill the epoch.  Items:
  kernel   device time per batch, HIP events, warm, `--runs` windows of 50 launches each with the three variants alternating
           inside every window round; reported as median / min / max over the windows:
             image_resample        the eval transform (Resize(256) + CenterCrop(256)) on the batch's frames
             image_augment_eval    mla_image_augment on the SAME descriptors with a full three-operation jitter: the
                                   difference to image_resample is the jitter's cost (second launch, staging round trip)
             image_augment_train   mla_image_augment on RandomResizedCrop boxes of the same frames (smaller crops: less to read)
  host     M3AEBatcher host samples/s (decode or cache read + draws + packing into pinned staging), 1/8/16 threads, no consumer
  step     MLATrainer(M3AEClassifier) samples/s: fed device-resident tensors, from the decoded cache and from JPEGs
           (M3AEBatcher + DeviceFeeder, train transform)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))

from mla_hip import (DeviceFeeder, M3AEBatcher, M3AEClassifier, MLATrainer, decode_images, image_descriptors,  # noqa: E402
                     jitter_descriptors, ops, resize_center_crop, sample_crop, sample_flip, sample_generator, sample_jitter)
from mla_hip.frames import make_lut  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def write_dataset(root, n, H, W):
    from PIL import Image
    rng = np.random.default_rng(0)
    text, visual = os.path.join(root, "text"), os.path.join(root, "visual")
    os.makedirs(text)
    os.makedirs(visual)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        n_tok = 20 + i % 200
        token = np.zeros((1, 256), dtype=np.int64)
        token[0, :n_tok] = rng.integers(1, 30000, n_tok)
        pm = np.ones((1, 256), dtype=np.float32)
        pm[0, :n_tok] = 0.0
        np.save(os.path.join(text, f"s{i}_token.npy"), token)
        np.save(os.path.join(text, f"s{i}_pm.npy"), pm)
        img = np.stack([(xx + 7 * i) % 256, (yy * 2 + i) % 256, (xx + yy) // 3 % 256], -1)
        img = np.clip(img + rng.integers(-12, 12, size=img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(visual, f"s{i}.jpg"), quality=90)
    return [f"s{i}" for i in range(n)], text, visual


def window(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def timed_epoch(tr, batches, warm):
    """samples/s over the steps after the first `warm` of one pass (one sync at the start of the timed window)."""
    n, t0 = 0, None
    for s, (token, pm, image, label, *_rest) in enumerate(batches):
        if s == warm:
            tr.join()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        tr.train_step(token, pm, image, label, s, 100)
        if t0 is not None:
            n += label.shape[0]
    tr.join()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--frame", default="384x512")
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--skip", default="", help="comma list of items to skip: kernel,host,step")
    a = ap.parse_args()
    H, W = (int(v) for v in a.frame.split("x"))
    skip = set(a.skip.split(",")) if a.skip else set()
    B, S = a.batch, 256
    if not torch.cuda.is_available():
        raise SystemExit("bench_m3ae_feed.py needs a GPU")

    if "kernel" not in skip:
        shapes = [(H, W)] * B
        e_desc, nbytes = image_descriptors(shapes, [(0, 0, H, W, 0)] * B, [resize_center_crop(H, W, S)] * B)
        boxes, jitters = [], []
        for i in range(B):
            g = sample_generator(0, 0, i)
            boxes.append(sample_crop(H, W, g) + (int(sample_flip(g)),))
            jitters.append(sample_jitter(g))
        t_desc, _ = image_descriptors(shapes, boxes, [(S, S, 0, 0)] * B)
        frames = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        eh, th, jh = torch.from_numpy(e_desc), torch.from_numpy(t_desc), torch.from_numpy(jitter_descriptors(jitters))
        ed, td, jd, lut = eh.cuda(), th.cuda(), jh.cuda(), make_lut().cuda()
        out = torch.empty((B, 3, 1, S, S), device="cuda")
        staging = torch.empty(B * S * S * 3, dtype=torch.uint8, device="cuda")
        partials = torch.empty(B * S, dtype=torch.int64, device="cuda")
        variants = {"image_resample": lambda: ops.image_resample(frames, ed, eh, lut, out, 1, 1),
                    "image_augment_eval": lambda: ops.image_augment(frames, ed, eh, jd, jh, lut, out, staging, partials),
                    "image_augment_train": lambda: ops.image_augment(frames, td, th, jd, jh, lut, out, staging, partials)}
        for fn in variants.values():
            for _ in range(5):
                fn()
        ms = {k: [] for k in variants}
        for _ in range(a.runs):                          # the variants alternate inside every round
            for k, fn in variants.items():
                ms[k].append(window(fn, 50))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            emit(item="kernel", kernel=k, images=B, frame=f"{H}x{W}", out=S, runs=a.runs, launches_per_run=50,
                 ms_median=round(med[k], 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                 ratio_to_image_resample=round(med[k] / med["image_resample"], 3))

    with tempfile.TemporaryDirectory() as tmp:
        base, text, visual = write_dataset(tmp, a.samples, H, W)
        cache = os.path.join(tmp, "cache")
        decode_images(visual, cache, base)
        names = (base * ((B * a.steps + len(base) - 1) // len(base)))[:B * a.steps]

        if "host" not in skip:
            for src in ("jpeg", "cache"):
                for threads in (1, 8, 16):
                    kw = {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}
                    nb = 5 if threads == 1 else max(a.steps, 8)
                    nm = (names * ((B * nb + len(names) - 1) // len(names)))[:B * nb]
                    fb = M3AEBatcher(nm, [0] * len(nm), B, text, threads=threads, pin=True, ring=2, **kw)
                    n, t0 = 0, None
                    for s, b in enumerate(fb):               # timed from batch 2 on: both pinned staging slots exist
                        if s == 2:
                            t0 = time.perf_counter()
                        if t0 is not None:
                            n += b[5].shape[0]
                    dt = time.perf_counter() - t0
                    fb.close()
                    emit(item="host", source=src, threads=threads, samples_per_s=round(n / dt, 1))

        if "step" not in skip:
            class Args:
                fusion_method, dataset, gs_flag, modulation = "concat", "Food101", True, "Normal"
            tr = MLATrainer(M3AEClassifier(Args(), depth=a.depth, seed=1))
            tr.keep_debug = False
            labels = [i % 101 for i in range(len(names))]
            g = torch.Generator(device="cuda").manual_seed(0)
            token = torch.randint(1, 30000, (B, 1, 256), device="cuda", generator=g)
            pm = (torch.arange(256, device="cuda")[None, :] >= torch.randint(8, 257, (B, 1), device="cuda", generator=g)).float().view(B, 1, 256)
            image = torch.randn((B, 3, S, S), device="cuda", generator=g)
            label = torch.randint(0, 101, (B,), device="cuda", generator=g)
            sps = timed_epoch(tr, [(token, pm, image, label)] * a.steps, a.warm)
            emit(item="step", source="device_tensors", batch=B, depth=a.depth, samples_per_s=round(sps, 1), ms_per_step=round(1e3 * B / sps, 2))
            for src, threads in (("cache", 1), ("cache", 16), ("jpeg", 16)):
                kw = {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}
                fb = M3AEBatcher(names, labels, B, text, threads=threads, pin=True, **kw)
                sps = timed_epoch(tr, DeviceFeeder(fb, depth=3), a.warm)
                fb.close()
                emit(item="step", source=src, batch=B, depth=a.depth, threads=threads, samples_per_s=round(sps, 1),
                     ms_per_step=round(1e3 * B / sps, 2))


if __name__ == "__main__":
    main()
