"""CAV-MAE batch feed: kernel times, host feed rates and the MLA step fed from the batcher (one JSON line per item).

    python scripts/bench_cav_feed.py [--batch 64] [--steps 8] [--frame 360x480] [--depth 12]

Synthetic JPEGs (smooth gradients + noise, PIL quality 90, the CREMA-D frame size) and fbank .npy files are written to a
temporary directory; `--samples` distinct clips are repeated to fill the epoch.  Items:
  kernel          mla_image_resample (batch frames -> 224, bicubic) and mla_fbank_augment (batch x 1024 x 128, every sample
                  augmented), HIP events, warm
  host            CAVBatcher host samples/s (decode or cache read + draws + packing into pinned staging), 1/8/16 threads, with
                  no consumer
  cpu_reference   the reference's per-sample CPU pipeline (PIL decode, bicubic Resize, CenterCrop, ToTensor, Normalize; fbank
                  masks, normalisation, noise, roll with torch ops), 16 threads
  step            MLATrainer(CAVClassifier) samples/s under Adam with the --cav_opti groups: fed device-resident tensors
                  (scripts/bench_cav.py's input), from the decoded cache and from JPEGs (CAVBatcher + DeviceFeeder, --cav_augnois)
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

from mla_hip import (CAVBatcher, CAVClassifier, DeviceFeeder, MLATrainer, cav_param_groups, decode_middle_frames,  # noqa: E402
                     fbank_descriptors, image_descriptors, ops, pick_middle_frame, resize_center_crop, sample_fbank_aug,
                     sample_generator)
from mla_hip.frames import MEAN, STD, make_lut  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def write_dataset(root, n, H, W, frames_per_clip=3):
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


def cpu_reference_sample(audio, visual, name, g):
    """CAVDataset.__getitem__ with --cav_augnois (dataset.py:296-325), restated with PIL + torch ops."""
    from PIL import Image
    fbank = torch.tensor(np.load(os.path.join(audio, name + ".npy")))
    f0, fw, t0, tw, s, roll = sample_fbank_aug(g)
    fbank[:, f0:f0 + fw] = 0
    fbank[t0:t0 + tw, :] = 0
    d = os.path.join(visual, name)
    im = Image.open(os.path.join(d, pick_middle_frame(d))).convert("RGB")
    fh, fw_, top, left = resize_center_crop(im.size[1], im.size[0], 224)
    im = im.resize((fw_, fh), Image.BICUBIC).crop((left, top, left + 224, top + 224))
    t = torch.from_numpy(np.array(im, np.uint8, copy=True)).permute(2, 0, 1).contiguous().float().div(255)
    t = t.sub_(torch.as_tensor(MEAN)[:, None, None]).div_(torch.as_tensor(STD)[:, None, None])
    fbank = (fbank - (-5.081)) / 4.4849
    fbank = fbank + torch.rand(fbank.shape[0], fbank.shape[1], generator=g) * s / 10
    return torch.roll(fbank, roll, 0), t


def timed(fn, reps):
    for _ in range(5):
        fn()
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
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--frame", default="360x480")
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--skip", default="", help="comma list of items to skip: kernel,host,cpu_reference,step")
    a = ap.parse_args()
    H, W = (int(v) for v in a.frame.split("x"))
    skip = set(a.skip.split(",")) if a.skip else set()
    B = a.batch
    with tempfile.TemporaryDirectory() as tmp:
        base, audio, visual = write_dataset(tmp, a.samples, H, W)
        cache = os.path.join(tmp, "cache")
        decode_middle_frames(visual, cache, base)
        names = (base * ((B * a.steps + len(base) - 1) // len(base)))[:B * a.steps]

        if "kernel" not in skip:
            shapes = [(H, W)] * B
            desc, nbytes = image_descriptors(shapes, [(0, 0, H, W, 0)] * B, [resize_center_crop(H, W, 224)] * B)
            frames = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
            dh = torch.from_numpy(desc)
            dd, lut = dh.cuda(), make_lut().cuda()
            out = torch.empty((B, 3, 1, 224, 224), device="cuda")
            ms = timed(lambda: ops.image_resample(frames, dd, dh, lut, out, 1, 1), 50)
            emit(item="kernel", kernel="image_resample", frames=B, frame=f"{H}x{W}", ms_per_batch=round(ms, 4),
                 read_mb=round(nbytes / 1e6, 1), write_mb=round(out.numel() * 4 / 1e6, 1),
                 gbps=round((nbytes + out.numel() * 4) / ms / 1e6, 1))
            x = torch.randn((B, 1024, 128), device="cuda") * 4.5 - 5.0
            y = torch.empty_like(x)
            fh = torch.from_numpy(fbank_descriptors([sample_fbank_aug(sample_generator(0, 0, i)) for i in range(B)], list(range(B))))
            fd = fh.cuda()
            ms = timed(lambda: ops.fbank_augment(x, y, fd, fh, -5.081, 4.4849, 0), 50)
            emit(item="kernel", kernel="fbank_augment", shape=[B, 1024, 128], ms_per_batch=round(ms, 4),
                 gbps=round(2 * x.numel() * 4 / ms / 1e6, 1))

        if "host" not in skip:
            for src in ("jpeg", "cache"):
                for threads in (1, 8, 16):
                    kw = {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}
                    nb = 5 if threads == 1 else max(a.steps, 8)
                    nm = (names * ((B * nb + len(names) - 1) // len(names)))[:B * nb]
                    fb = CAVBatcher(nm, [0] * len(nm), B, audio, augnois=True, threads=threads, pin=True, ring=2, **kw)
                    n, t0 = 0, None
                    for s, b in enumerate(fb):               # timed from batch 2 on: both pinned staging slots exist
                        if s == 2:
                            t0 = time.perf_counter()
                        if t0 is not None:
                            n += b[4].shape[0]
                    dt = time.perf_counter() - t0
                    fb.close()
                    emit(item="host", source=src, threads=threads, samples_per_s=round(n / dt, 1))

        if "cpu_reference" not in skip:
            todo = names[:B * 2]
            with ThreadPoolExecutor(16) as pool:
                list(pool.map(lambda nm: cpu_reference_sample(audio, visual, nm, torch.Generator().manual_seed(1)), todo[:32]))
                t0 = time.perf_counter()
                list(pool.map(lambda inm: cpu_reference_sample(audio, visual, inm[1], torch.Generator().manual_seed(inm[0])), enumerate(todo)))
                dt = time.perf_counter() - t0
            emit(item="cpu_reference", threads=16, samples_per_s=round(len(todo) / dt, 1))

        if "step" not in skip:
            class Args:
                fusion_method, dataset, gs_flag, modulation, lorb = "concat", "CREMAD", True, "Normal", "large"
            model = CAVClassifier(Args(), depth=a.depth, seed=1)
            tr = MLATrainer(model, optimizer="adam", betas=(0.95, 0.999), weight_decay=5e-7, param_groups=cav_param_groups(model, 1e-3))
            tr.keep_debug = False
            labels = [i % 6 for i in range(len(names))]
            g = torch.Generator(device="cuda").manual_seed(0)
            spec = torch.randn((B, 1024, 128), device="cuda", generator=g)
            image = torch.randn((B, 3, 224, 224), device="cuda", generator=g)
            label = torch.randint(0, 6, (B,), device="cuda", generator=g)
            sps = timed_epoch(tr, [(spec, image, label)] * a.steps, a.warm)
            emit(item="step", source="device_tensors", batch=B, depth=a.depth, samples_per_s=round(sps, 1), ms_per_step=round(1e3 * B / sps, 2))
            for src, threads in (("cache", 1), ("cache", 16), ("jpeg", 16)):
                kw = {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}
                fb = CAVBatcher(names, labels, B, audio, augnois=True, threads=threads, pin=True, **kw)
                sps = timed_epoch(tr, DeviceFeeder(fb, depth=3), a.warm)
                fb.close()
                emit(item="step", source=src, batch=B, depth=a.depth, threads=threads, samples_per_s=round(sps, 1),
                     ms_per_step=round(1e3 * B / sps, 2))


if __name__ == "__main__":
    main()
