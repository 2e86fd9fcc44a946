"""M3AEDataset batches (dataset/dataset.py:327-480; Food-101 / MVSA / CUB, `--lorb m3ae`) -> M3AEClassifier inputs on the device.

The reference reads, per sample, `<text>/<name>_token.npy`, `<text>/<name>_pm.npy` and the image `<visual>/<name>.jpg`, and
transforms the image on the CPU:

    train (dataset.py:401-412)   timm create_transform(256, is_training=True, color_jitter=True, auto_augment=None, "bicubic",
                                 re_prob=0) = RandomResizedCropAndInterpolation(256, (0.08, 1), (3/4, 4/3), BICUBIC),
                                 RandomHorizontalFlip(0.5), ColorJitter(1.0, 1.0, 1.0), ToTensor(), Normalize(mean, std)
    eval  (dataset.py:413-420)   Resize(256, BICUBIC), CenterCrop(256), ToTensor(), Normalize(mean, std)

Here the host only decodes (or memcpys an image `decode_images` decoded once), draws the crop box, the flip and the jitter and
packs descriptors; the work runs in csrc/frames.hip behind the batch's copies:

    mla_image_augment    crop -> Pillow-exact bicubic resize -> flip -> Pillow's ImageEnhance.Brightness / Contrast / Color in the
                         drawn order -> LUT (ToTensor + Normalize); two launches (contrast needs the image's mean luma)
    mla_image_resample   the eval transform: what CAVBatcher(out_size=256, train=False) runs, bit for bit

The transform is pinned to Pillow (bit for bit: tests/jitter_model.py, tests/golden/m3ae_feed_small.npz) plus the restated
sampling of timm 0.4.5 / torchvision 0.9.1; neither library is needed.  `color_jitter=True` becomes (float(True),) * 3 in timm,
so every factor is uniform in [max(0, 1 - 1), 1 + 1] = [0, 2] and there is no hue.  ColorJitter draws randperm(4), then the
brightness, contrast and saturation factors; slot 3 (hue) of the permutation is empty.  The crop box is frames.sample_crop
(torchvision's RandomResizedCrop.get_params): timm's copy differs only in accepting w == 0 or h == 0 (`w <= img_w and h <=
img_h` without `0 <`), which can only happen on images a few pixels wide and would crash PIL's resize; the existing sampler is
kept.  Every draw is a function of (seed, epoch, dataset index): batches do not depend on thread count, ring depth or rank.
(The reference draws from per-worker global streams, so its own sequence is not reproducible; the distributions and the
algorithm are what is matched.)  The reference's token noise is dead code (`self.noise = False`) and is not reproduced.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .cav_feed import ResizeCenterCrop
from .frames import (MAX_THREADS, MEAN, RATIO, SCALE, STD, Batcher, ImagePart, Placement, SampleKey, _cache_path, decode_jpeg,
                     sample_crop, sample_flip, sample_generator, token_part)

OUT_SIZE = 256                                        # dataset.py:402, 415-416
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2            # operation ids of mla_image_augment = torchvision ColorJitter's fn_id
JITTER_COLS = 7
Jitter = Tuple[Tuple[int, ...], Tuple[float, float, float]]
NO_JITTER: Jitter = ((), (1.0, 1.0, 1.0))


def sample_jitter(g: torch.Generator, brightness: float = 1.0, contrast: float = 1.0, saturation: float = 1.0) -> Jitter:
    """torchvision 0.9.1 ColorJitter(brightness, contrast, saturation) on `g`: (operation ids in the order they are applied,
    (brightness, contrast, saturation factor)).  Draws: randperm(4), then each factor as an fp32 uniform in
    [max(0, 1 - strength), 1 + strength].  A strength of 0 is torchvision's None: no draw, the operation is dropped (its factor
    is reported as 1.0).  Entry 3 of the permutation is hue, which the reference does not set."""
    perm = torch.randperm(4, generator=g).tolist()
    factors = []
    for strength in (brightness, contrast, saturation):
        if strength < 0:
            raise ValueError("jitter strengths must be non-negative")
        if strength == 0:
            factors.append(None)
        else:
            factors.append(torch.empty(1).uniform_(max(0.0, 1.0 - strength), 1.0 + strength, generator=g).item())
    order = tuple(op for op in perm if op < 3 and factors[op] is not None)
    return order, tuple(1.0 if f is None else f for f in factors)


def jitter_descriptors(jitters: Sequence[Optional[Jitter]]) -> np.ndarray:
    """int64 (N, 7) rows (n_ops, op0, op1, op2, brightness bits, contrast bits, saturation bits) from sample_jitter results
    (None, the image of a transform that draws no jitter, counts as NO_JITTER); unused operation slots hold -1, the bits are the
    patterns of fp32(factor) (Pillow's blend takes a C float)."""
    desc = np.zeros((len(jitters), JITTER_COLS), dtype=np.int64)
    for n, (order, factors) in enumerate(j or NO_JITTER for j in jitters):
        desc[n, 0] = len(order)
        desc[n, 1:4] = tuple(order) + (-1,) * (3 - len(order))
        desc[n, 4:7] = np.asarray(factors, dtype=np.float32).view(np.uint32)
    return desc


def decode_images(visual_feature_path: str, out_path: str, names: Sequence[str], threads: int = MAX_THREADS) -> int:
    """frames.decode_frames for datasets whose image is the single file <visual>/<name>.jpg: decode each once with PIL into
    <out_path>/<name>/0.npy (uint8 HWC).  M3AEBatcher(frame_cache=out_path) then gives batches bit-identical to the JPEG source
    with a memcpy per image instead of a decode.  Returns the number of files written."""
    def one(name):
        os.makedirs(os.path.join(out_path, name), exist_ok=True)
        np.save(_cache_path(out_path, name, 0), decode_jpeg(os.path.join(visual_feature_path, name + ".jpg")))
        return 1
    with ThreadPoolExecutor(max(1, min(int(threads), MAX_THREADS))) as pool:
        return sum(pool.map(one, names))


def image_path(visual: str, name: str, T: int = 1) -> List[str]:
    """Frame source of M3AEDataset for frames.ImagePart: the flat file <visual>/<name>.jpg."""
    return [os.path.join(visual, name + ".jpg")]


class TimmTrain:
    """Transform for frames.ImagePart: timm's train transform on one image.  Crop, flip and jitter draws in the transform's
    order, the crop resized to size x size (so the CenterCrop window is the whole resize); mla_image_augment."""
    cols, kernel, table = 12, "image_augment", staticmethod(ResizeCenterCrop.table)

    def __init__(self, size: int, scale: Sequence[float], ratio: Sequence[float], jitter: Sequence[float]):
        self.size, self.scale, self.ratio, self.jitter = int(size), tuple(scale), tuple(ratio), tuple(jitter)

    def place(self, shapes: Sequence[Tuple[int, int]], key: SampleKey) -> List[Placement]:
        (H, W), = shapes
        g = sample_generator(*key)
        crop = sample_crop(H, W, g, self.scale, self.ratio) + (int(sample_flip(g)),)
        return [Placement(crop, (self.size, self.size, 0, 0), sample_jitter(g, *self.jitter))]


def timm_image_part(visual_feature_path: Optional[str], frame_cache: Optional[str], paths, train: bool, out_size: int, scale, ratio,
                    color_jitter, mean, std, present=None) -> ImagePart:
    """The image part of M3AEDataset and Modal3Dataset: TimmTrain when `train`, else Resize(out) + CenterCrop(out); the jitter
    table is part of the host tuple either way."""
    cj = tuple(color_jitter) if isinstance(color_jitter, (list, tuple)) else (float(color_jitter),) * 3
    if len(cj) != 3 or min(cj) < 0:
        raise ValueError("color_jitter: one non-negative strength, or three (brightness, contrast, saturation)")
    transform = TimmTrain(out_size, scale, ratio, [float(v) for v in cj]) if train else ResizeCenterCrop(out_size)
    return ImagePart(visual_feature_path, frame_cache, paths, 1, transform, out_size, mean, std, jitter_table=jitter_descriptors,
                     present=present)


class M3AEBatcher(Batcher):
    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, text_feature_path: str,
                 visual_feature_path: Optional[str] = None, frame_cache: Optional[str] = None, train: bool = True, seed: int = 0,
                 epoch: int = 0, threads: int = 8, ring: int = 4, out_size: int = OUT_SIZE, scale: Sequence[float] = SCALE,
                 ratio: Sequence[float] = RATIO, color_jitter=1.0, mean: Sequence[float] = MEAN, std: Sequence[float] = STD,
                 drop_last: bool = False, pin: Optional[bool] = None):
        """M3AEDataset batches from the token / padding-mask .npy files and either the JPEG images (`visual_feature_path`) or a
        decode_images cache (`frame_cache`), on frames.Batcher's loop, staging ring, `copied()` fence and `device_step()` hook.
        Yields host tuples (token, padding_mask, frames uint8 (capacity,), image_desc int64 (B, 12), jitter_desc int64 (B, 7),
        label, idx); through a DeviceFeeder the device tuple is (token (B, 1, 256) int64, padding_mask (B, 1, 256) fp32,
        image (B, 3, out, out) fp32, label, idx): M3AEDataset.__getitem__'s tuple, what M3AEClassifier / MLATrainer take.
        `color_jitter`: one strength for brightness, contrast and saturation, or three (timm's convention); 0 drops the
        operation.  train=False: Resize(out) + CenterCrop(out), no draws, no jitter."""
        self.text = text_feature_path
        images = timm_image_part(visual_feature_path, frame_cache, image_path, train, out_size, scale, ratio, color_jitter, mean, std)
        super().__init__(names, labels, batch_size, [images, token_part(text_feature_path)],
                         ("token", "pm", "frames", "desc", "jdesc", "label", "idx"), ("token", "pm", "image", "label", "idx"),
                         seed=seed, epoch=epoch, threads=threads, ring=ring, pin=pin, drop_last=drop_last)
