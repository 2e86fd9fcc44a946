"""Writes tests/golden/frames_small.npz: seeded uint8 RGB frames of mixed sizes, crop descriptors and PIL's uint8 results of
crop -> resize(BILINEAR) -> optional FLIP_LEFT_RIGHT (torchvision's RandomResizedCrop / Resize + RandomHorizontalFlip on PIL
images, dataset/dataset.py:128-140).  PIL + numpy only.  Run from the repository root: python tests/golden/make_golden_frames.py

Groups (one kernel launch each):
  g64   out 64 x 48 (H x W): full-frame upscale, downscale crops (one > 2x), an upscale crop, flips, the sampler's central
        fallback box of a 20 x 200 frame
  g224  out 224 x 224: an identity crop (exactly 224 x 224, flipped) of a 240 x 232 frame
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def fallback_box(H, W, ratio=(3 / 4, 4 / 3)):
    """(top, left, h, w) of RandomResizedCrop's central fallback (taken when its 10 tries all fail)."""
    r = W / H
    if r < min(ratio):
        w, h = W, int(round(W / min(ratio)))
    elif r > max(ratio):
        h, w = H, int(round(H * max(ratio)))
    else:
        h, w = H, W
    return (H - h) // 2, (W - w) // 2, h, w


def pil(frame, top, left, h, w, flip, OH, OW):
    im = Image.fromarray(frame).crop((left, top, left + w, top + h)).resize((OW, OH), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def main():
    rng = np.random.default_rng(20261016)
    shapes = [(37, 53), (150, 110), (20, 200), (240, 232)]
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
    offs = np.cumsum([0] + [f.size for f in frames])[:-1]
    packed = np.concatenate([f.reshape(-1) for f in frames])
    fb = fallback_box(20, 200)
    cases = {
        "g64": ((64, 48), [(0, 0, 0, 37, 53, 0),          # full frame, upscale (eval Resize)
                           (1, 10, 7, 120, 90, 1),        # downscale crop, flipped
                           (1, 0, 0, 150, 110, 0),        # downscale > 2x in both axes
                           (1, 3, 5, 40, 30, 1),          # upscale crop, flipped
                           (2,) + fb + (0,),              # the sampler's fallback box
                           (0, 30, 40, 7, 13, 1)]),       # tiny crop at the frame's corner
        "g224": ((224, 224), [(3, 8, 4, 224, 224, 1)]),   # identity size, flipped
    }
    out = {"frames": packed}
    for g, ((OH, OW), rows) in cases.items():
        desc = np.array([(offs[f], shapes[f][0], shapes[f][1], t, l, h, w, fl) for f, t, l, h, w, fl in rows], dtype=np.int64)
        res = np.stack([pil(frames[f], t, l, h, w, fl, OH, OW) for f, t, l, h, w, fl in rows])
        out[f"desc_{g}"], out[f"out_{g}"] = desc, res
    path = os.path.join(HERE, "frames_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
