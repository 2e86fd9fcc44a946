"""Writes tests/golden/cav_feed_small.npz: seeded uint8 RGB frames of mixed sizes, 12-column image descriptors and PIL's uint8
results of crop -> resize(BICUBIC) to the Resize(size) shape -> CenterCrop(size) window -> optional FLIP_LEFT_RIGHT
(torchvision's Resize(size, BICUBIC) + CenterCrop(size) on PIL images, dataset/dataset.py:251-256 and, at 256, 413-420).
PIL + numpy only.  Run from the repository root: python tests/golden/make_golden_cav_feed.py

Descriptor row: byte offset, H, W, crop top, crop left, crop h, crop w, flip, full_h, full_w, win_top, win_left.
Groups (one kernel launch each):
  w32   window 32 x 32: landscape and portrait downscales (windows off centre by a half-to-even rounding), an upscale of a
        17 x 23 crop, a flipped crop box, a 0 / 255 checkerboard (the negative lobes overshoot and are clipped), a frame whose
        short side is already 32 (identity pass along that axis)
  w224  window 224 x 224: a 240 x 232 frame (231 x 224 resized, window top 4) and the 37 x 53 frame upscaled 6x
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def resize_center_crop(H, W, size):
    """torchvision Resize(size) + CenterCrop(size): (full_h, full_w, win_top, win_left)."""
    if W <= H:
        ow, oh = size, int(size * H / W)
    else:
        oh, ow = size, int(size * W / H)
    return oh, ow, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


def pil(frame, top, left, h, w, flip, full_h, full_w, win_top, win_left, size):
    im = Image.fromarray(frame).crop((left, top, left + w, top + h)).resize((full_w, full_h), Image.BICUBIC)
    im = im.crop((win_left, win_top, win_left + size, win_top + size))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im)


def main():
    rng = np.random.default_rng(20261018)
    shapes = [(37, 53), (150, 110), (61, 47), (240, 232), (32, 75)]
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in shapes]
    yy, xx = np.mgrid[0:61, 0:47]
    frames[2] = np.repeat(((((yy // 3) + (xx // 2)) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    offs = np.cumsum([0] + [f.size for f in frames])[:-1]
    packed = np.concatenate([f.reshape(-1) for f in frames])
    # (frame, top, left, h, w, flip)
    cases = {
        "w32": (32, [(0, 0, 0, 37, 53, 0),            # landscape downscale: 32 x 45, window left round(6.5) = 6
                     (1, 0, 0, 150, 110, 0),          # portrait downscale > 3x: 43 x 32, window top round(5.5) = 6
                     (0, 10, 20, 17, 23, 0),          # upscale of a crop
                     (1, 7, 9, 120, 90, 1),           # crop box, flipped
                     (2, 0, 0, 61, 47, 0),            # 0 / 255 checkerboard
                     (4, 0, 0, 32, 75, 1)]),          # short side already 32, flipped
        "w224": (224, [(3, 0, 0, 240, 232, 0),        # 231 x 224, window top round(3.5) = 4
                       (0, 0, 0, 37, 53, 0)]),        # 6x upscale: 224 x 320, window left 48
    }
    out = {"frames": packed}
    for g, (size, rows) in cases.items():
        desc, res = [], []
        for f, t, l, h, w, fl in rows:
            win = resize_center_crop(h, w, size)
            desc.append((offs[f], shapes[f][0], shapes[f][1], t, l, h, w, fl) + win)
            res.append(pil(frames[f], t, l, h, w, fl, *win, size))
        out[f"desc_{g}"], out[f"out_{g}"] = np.array(desc, dtype=np.int64), np.stack(res)
    path = os.path.join(HERE, "cav_feed_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
