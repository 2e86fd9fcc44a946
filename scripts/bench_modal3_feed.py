"""Modal3 (IEMOCAP, three-modality) batch feed: the assemble kernel, host feed rates and the MLA step fed from the batcher (one JSON
line per item).

    python scripts/bench_modal3_feed.py [--batch 32] [--steps 8] [--frame 384x512] [--depth 12] [--runs 7]

Synthetic JPEG frame directories (smooth gradients + noise, PIL quality 90), fbank and token / padding-mask .npy files are written
to a temporary directory; `--samples` distinct samples are repeated to fill the epoch.  Mask rates 0, 0.3 and 0.7 (all present;
the rejection loop; one modality per sample), drawn by random_mask.  Items:
  kernel   mla_modal3_assemble alone, device time per batch, HIP events, warm, `--runs` windows of 50 launches with the three rates
           alternating inside every round; median / min / max over the windows, the bytes the launch moves (a present image is
           read and written, every absent row is written, the table is read) and the resulting GB/s.  The launch is idempotent
           (it zeroes rows in place), so repeating it measures the same work.
  host     Modal3Batcher host batches/s (decode or cache read + fbank / token reads + draws + packing into pinned staging), no
           consumer, JPEG source and decoded cache, 1 and 8 threads, at the three rates
  step     MLATrainer(Modal3Classifier) samples/s: fed device-resident tensors (the step of scripts/bench_modal3.py), then from the
           batcher through a DeviceFeeder (train transform) from the cache and from JPEGs at rate 0, and from the cache at the
           other rates, in the same process
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

from mla_hip import (DeviceFeeder, MLATrainer, Modal3Batcher, Modal3Classifier, decode_middle_frames, mask_descriptors, ops,  # noqa: E402
                     random_mask)

RATES = (0.0, 0.3, 0.7)
S, T, F, L = 256, 1024, 128, 256


def emit(**kw):
    print(json.dumps(kw), flush=True)


def write_dataset(root, n, H, W, n_frames=3):
    from PIL import Image
    rng = np.random.default_rng(0)
    text, audio, visual = (os.path.join(root, d) for d in ("text", "audio", "visual"))
    for d in (text, audio, visual):
        os.makedirs(d)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        n_tok = 20 + i % 200
        token = np.zeros((1, L), dtype=np.int64)
        token[0, :n_tok] = rng.integers(1, 30000, n_tok)
        pm = np.ones((1, L), dtype=np.float32)
        pm[0, :n_tok] = 0.0
        np.save(os.path.join(text, f"s{i}_token.npy"), token)
        np.save(os.path.join(text, f"s{i}_pm.npy"), pm)
        np.save(os.path.join(audio, f"s{i}.npy"), (rng.standard_normal((T, F)) * 4.4849 - 5.081).astype(np.float32))
        os.makedirs(os.path.join(visual, f"s{i}"))
        for t in range(n_frames):
            img = np.stack([(xx + 7 * i + 3 * t) % 256, (yy * 2 + i) % 256, (xx + yy) // 3 % 256], -1)
            img = np.clip(img + rng.integers(-12, 12, size=img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(visual, f"s{i}", f"{t:04d}.jpg"), quality=90)
    return [f"s{i}" for i in range(n)], text, audio, visual


def window(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def assemble_bytes(table):
    """Bytes one launch moves for a mask table (B, 4): present images read + written, absent rows written, the table read."""
    img, spec, tok, pm = 3 * S * S * 4, T * F * 4, L * 8, L * 4
    a, i, t = (table[:, c] for c in range(3))
    return int((i * 2 * img + (1 - i) * img + (1 - a) * spec + (1 - t) * (tok + pm)).sum()) + table.size * 8


def timed_epoch(tr, batches, warm):
    """samples/s over the steps after the first `warm` of one pass (one sync at the start of the timed window)."""
    n, t0 = 0, None
    for s, (token, pm, image, spec, label, *_rest) in enumerate(batches):
        if s == warm:
            tr.join()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        tr.train_step(token, pm, image, spec, label, s, 100)
        if t0 is not None:
            n += label.shape[0]
    tr.join()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--frame", default="384x512")
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--skip", default="", help="comma list of items to skip: kernel,host,step")
    a = ap.parse_args()
    H, W = (int(v) for v in a.frame.split("x"))
    skip = set(a.skip.split(",")) if a.skip else set()
    B = a.batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_modal3_feed.py needs a GPU")

    if "kernel" not in skip:
        variants, meta = {}, {}
        for rate in RATES:
            table = mask_descriptors(random_mask(3, B, rate, np.random.RandomState(0)))
            P = int(table[:, 1].sum())
            th = torch.from_numpy(table)
            buf = dict(compact=torch.randn((P, 3, S, S), device="cuda") if P else None, spec=torch.randn((B, T, F), device="cuda"),
                       token=torch.randint(1, 30000, (B, 1, L), device="cuda"), pm=torch.zeros((B, 1, L), device="cuda"),
                       td=th.cuda(), th=th, out=torch.empty((B, 3, S, S), device="cuda"))
            variants[rate] = (lambda b: lambda: ops.modal3_assemble(b["compact"], b["spec"], b["token"], b["pm"], b["td"], b["th"], b["out"]))(buf)
            meta[rate] = (P, assemble_bytes(table), table[:, :3].mean())
        for fn in variants.values():
            for _ in range(5):
                fn()
        ms = {k: [] for k in variants}
        for _ in range(a.runs):                          # the rates alternate inside every round
            for k, fn in variants.items():
                ms[k].append(window(fn, 50))
        for k, v in ms.items():
            med, (P, nbytes, share) = statistics.median(v), meta[k]
            emit(item="kernel", kernel="modal3_assemble", mask_rate=k, batch=B, images_present=P, share_of_ones=round(float(share), 4),
                 runs=a.runs, launches_per_run=50, ms_median=round(med, 5), ms_min=round(min(v), 5), ms_max=round(max(v), 5),
                 mbytes_moved=round(nbytes / 1e6, 2), gbytes_per_s=round(nbytes / med / 1e6, 1))

    with tempfile.TemporaryDirectory() as tmp:
        base, text, audio, visual = write_dataset(tmp, a.samples, H, W)
        cache = os.path.join(tmp, "cache")
        decode_middle_frames(visual, cache, base)
        names = (base * ((B * a.steps + len(base) - 1) // len(base)))[:B * a.steps]
        source = lambda src: {"visual_feature_path": visual} if src == "jpeg" else {"frame_cache": cache}

        if "host" not in skip:
            for src in ("jpeg", "cache"):
                for threads in (1, 8):
                    for rate in RATES:
                        nb = 5 if threads == 1 else max(a.steps, 8)
                        nm = (names * ((B * nb + len(names) - 1) // len(names)))[:B * nb]
                        fb = Modal3Batcher(nm, [0] * len(nm), B, text, audio, threads=threads, pin=True, ring=2, mask_percent=rate,
                                           **source(src))
                        n, t0 = 0, None
                        for s, b in enumerate(fb):               # timed from batch 2 on: both pinned staging slots exist
                            if s == 2:
                                t0 = time.perf_counter()
                            if t0 is not None:
                                n += 1
                        dt = time.perf_counter() - t0
                        fb.close()
                        emit(item="host", source=src, threads=threads, mask_rate=rate, batch=B, batches_per_s=round(n / dt, 2),
                             samples_per_s=round(n * B / dt, 1))

        if "step" not in skip:
            class Args:
                fusion_method, dataset, gs_flag, modulation, modal3 = "concat", "IEMOCAP", True, "Normal", True
            tr = MLATrainer(Modal3Classifier(Args(), depth=a.depth, seed=1))
            tr.keep_debug = False
            labels = [i % 4 for i in range(len(names))]
            g = torch.Generator(device="cuda").manual_seed(0)
            token = torch.randint(0, 30522, (B, 1, L), device="cuda", generator=g)
            pm = (torch.arange(L, device="cuda")[None, :] >= torch.randint(8, 257, (B, 1), device="cuda", generator=g)).float().view(B, 1, L)
            image = torch.randn((B, 3, S, S), device="cuda", generator=g)
            spec = torch.randn((B, T, F), device="cuda", generator=g) * 4.4849 - 5.081
            label = torch.randint(0, 4, (B,), device="cuda", generator=g)
            tensors = [(token, pm, image, spec, label)] * a.steps

            def fed(src, threads, rate):
                fb = Modal3Batcher(names, labels, B, text, audio, threads=threads, pin=True, mask_percent=rate, **source(src))
                sps = timed_epoch(tr, DeviceFeeder(fb, depth=3), a.warm)
                fb.close()
                return sps
            runs = [("device_tensors", None, None, lambda: timed_epoch(tr, tensors, a.warm)),
                    ("cache", 1, 0.0, lambda: fed("cache", 1, 0.0)), ("jpeg", 8, 0.0, lambda: fed("jpeg", 8, 0.0)),
                    ("device_tensors", None, None, lambda: timed_epoch(tr, tensors, a.warm)),       # again: the spread of the yardstick
                    ("cache", 1, 0.3, lambda: fed("cache", 1, 0.3)), ("cache", 1, 0.7, lambda: fed("cache", 1, 0.7)),
                    ("cache", 1, 0.0, lambda: fed("cache", 1, 0.0))]
            for src, threads, rate, fn in runs:
                sps = fn()
                emit(item="step", source=src, batch=B, depth=a.depth, threads=threads, mask_rate=rate, samples_per_s=round(sps, 1),
                     ms_per_step=round(1e3 * B / sps, 2))


if __name__ == "__main__":
    main()
