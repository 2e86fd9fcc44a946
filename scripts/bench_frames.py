"""CREMA-D frame pipeline: kernel time, host feed rates and the end-to-end MLA step fed from frames (one JSON line per item).

    python scripts/bench_frames.py [--batch 64] [--steps 12] [--frame 360x480]

Synthetic JPEGs (smooth gradients + noise, PIL quality 90, the CREMA-D frame size) and fbank .npy files are written to a
temporary directory; `--samples` distinct clips are repeated to fill the epoch.  Items:
  kernel          mla_frames_resample for batch x 3 frames (RandomResizedCrop boxes), HIP events, warm
  host            FrameBatcher host frames/s (decode or cache read + draws + packing into pinned staging), 1/8/16 threads,
                  with no consumer (the staging ring is allocated before the timed window)
  cpu_reference   the reference's per-frame CPU pipeline (PIL decode, crop, resize, flip, ToTensor, Normalize), 16 threads
  step            MLATrainer samples/s fed from JPEGs, from the decoded cache (FrameBatcher + DeviceFeeder) and from
                  device-resident tensors (bench.py's input)
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd"))

from mla_hip import AVClassifier, DeviceFeeder, FrameBatcher, MLATrainer, decode_frames, ops  # noqa: E402
from mla_hip.frames import MEAN, STD, frame_descriptors, make_lut, pick_frames, sample_augment, sample_generator  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def write_dataset(root, n, H, W, frames_per_clip=6):
    from PIL import Image
    rng = np.random.default_rng(0)
    audio, visual = os.path.join(root, "audio"), os.path.join(root, "visual")
    os.makedirs(audio)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        np.save(os.path.join(audio, f"c{i}.npy"), (rng.standard_normal((1024, 128)) * 4.5 - 5.0).astype(np.float32))
        d = os.path.join(visual, f"c{i}")
        os.makedirs(d)
        for f in range(frames_per_clip):
            img = np.stack([(xx + 7 * f + i) % 256, (yy * 2 + i) % 256, (xx + yy) // 3 % 256], -1)
            img = np.clip(img + rng.integers(-12, 12, size=img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f"{f:05d}.jpg"), quality=90)
    return [f"c{i}" for i in range(n)], audio, visual


def cpu_reference_frame(path, g):
    """dataset.py:146-147 with the training transform, restated with PIL + torch ops (torchvision's own code paths)."""
    from PIL import Image
    from mla_hip.frames import sample_crop, sample_flip
    im = Image.open(path).convert("RGB")
    top, left, h, w = sample_crop(im.size[1], im.size[0], g)
    im = im.crop((left, top, left + w, top + h)).resize((224, 224), Image.BILINEAR)
    if sample_flip(g):
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    t = torch.from_numpy(np.array(im, np.uint8, copy=True)).permute(2, 0, 1).contiguous().float().div(255)
    return t.sub_(torch.as_tensor(MEAN)[:, None, None]).div_(torch.as_tensor(STD)[:, None, None])


def make_trainer():
    class Args:
        fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"
    tr = MLATrainer(AVClassifier(Args(), seed=0))
    tr.keep_debug = False
    return tr


def timed_epoch(tr, batches, warm):
    """samples/s over the steps after the first `warm` of one pass (one sync at the start of the timed window)."""
    n, t0 = 0, None
    for s, (spec, image, label, *_rest) in enumerate(batches):
        if s == warm:
            tr.join()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        tr.train_step(spec, image, label, s, 100)
        if t0 is not None:
            n += label.shape[0]
    tr.join()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--frame", default="360x480")
    ap.add_argument("--skip", default="", help="comma list of items to skip: kernel,host,cpu_reference,step")
    a = ap.parse_args()
    H, W = (int(v) for v in a.frame.split("x"))
    skip = set(a.skip.split(",")) if a.skip else set()
    B, T = a.batch, 3
    with tempfile.TemporaryDirectory() as tmp:
        base, audio, visual = write_dataset(tmp, a.samples, H, W)
        cache = os.path.join(tmp, "cache")
        decode_frames(visual, cache, base)
        names = (base * ((B * a.steps + len(base) - 1) // len(base)))[:B * a.steps]

        if "kernel" not in skip:
            shapes = [(H, W)] * (B * T)
            boxes = []
            for i in range(B):
                boxes += sample_augment(shapes[:T], sample_generator(0, 0, i), True)
            desc, nbytes = frame_descriptors(shapes, boxes)
            frames = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
            dh = torch.from_numpy(desc)
            dd, lut = dh.cuda(), make_lut().cuda()
            out = torch.empty((B, 3, T, 224, 224), device="cuda")
            for _ in range(5):
                ops.frames_resample(frames, dd, dh, lut, out, T)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            reps = 50
            ev[0].record()
            for _ in range(reps):
                ops.frames_resample(frames, dd, dh, lut, out, T)
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / reps
            emit(item="kernel", frames=B * T, frame=f"{H}x{W}", ms_per_batch=round(ms, 4),
                 read_mb=round(nbytes / 1e6, 1), write_mb=round(out.numel() * 4 / 1e6, 1),
                 gbps=round((nbytes + out.numel() * 4) / ms / 1e6, 1))

        if "host" not in skip:
            for src in ("jpeg", "cache"):
                for threads in (1, 8, 16):
                    kw = {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}
                    nb = 5 if threads == 1 else max(a.steps, 8)
                    fb = FrameBatcher(names[:B * nb], [0] * (B * nb), B, audio, threads=threads, pin=True, ring=2, **kw)
                    n, t0 = 0, None
                    for s, b in enumerate(fb):               # timed from batch 2 on: both pinned staging slots exist
                        if s == 2:
                            t0 = time.perf_counter()
                        if t0 is not None:
                            n += b[3].shape[0]
                    dt = time.perf_counter() - t0
                    fb.close()
                    emit(item="host", source=src, threads=threads, frames_per_s=round(n * T / dt, 1),
                         samples_per_s=round(n / dt, 1))

        if "cpu_reference" not in skip:
            paths = []
            for nm in names[:B * 2]:
                d = os.path.join(visual, nm)
                paths += [os.path.join(d, f) for f in pick_frames(d)]
            with ThreadPoolExecutor(16) as pool:
                list(pool.map(lambda p: cpu_reference_frame(p, torch.Generator().manual_seed(1)), paths[:32]))
                t0 = time.perf_counter()
                list(pool.map(lambda ip: cpu_reference_frame(ip[1], torch.Generator().manual_seed(ip[0])), enumerate(paths)))
                dt = time.perf_counter() - t0
            emit(item="cpu_reference", threads=16, frames_per_s=round(len(paths) / dt, 1))

        if "step" not in skip:
            labels = [i % 6 for i in range(len(names))]
            tr = make_trainer()
            g = torch.Generator(device="cuda").manual_seed(0)
            spec = torch.randn((B, 1024, 128), device="cuda", generator=g)
            image = torch.randn((B, 3, T, 224, 224), device="cuda", generator=g)
            label = torch.randint(0, 6, (B,), device="cuda", generator=g)
            sps = timed_epoch(tr, [(spec, image, label)] * a.steps, a.warm)
            emit(item="step", source="device_tensors", batch=B, samples_per_s=round(sps, 1))
            for src, threads in (("cache", 1), ("cache", 16), ("jpeg", 16)):
                kw = {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}
                fb = FrameBatcher(names, labels, B, audio, threads=threads, pin=True, **kw)
                sps = timed_epoch(tr, DeviceFeeder(fb, depth=3), a.warm)
                fb.close()
                emit(item="step", source=src, batch=B, threads=threads, samples_per_s=round(sps, 1))


if __name__ == "__main__":
    main()
