"""Writes tests/golden/m3ae_feed_small.npz: seeded uint8 RGB images up to 64 x 64, 12-column image descriptors, 7-column jitter
descriptors and PILLOW'S OWN uint8 results of crop -> resize((40, 40), BICUBIC) -> optional FLIP_LEFT_RIGHT -> ImageEnhance
.Brightness / .Contrast / .Color in the listed order (timm's train transform of dataset/dataset.py:401-412 up to ToTensor).
PIL + numpy, and tests/jitter_model.py for the checks below.  Run from the repository root:
    python tests/golden/make_golden_m3ae_feed.py

Image descriptor row: byte offset, H, W, crop top, crop left, crop h, crop w, flip, 40, 40, 0, 0.
Jitter descriptor row: n_ops, op0, op1, op2 (-1 = unused), then the fp32 bit patterns of the brightness, contrast and saturation
factors; operation ids 0 = brightness, 1 = contrast, 2 = saturation.
40 rows are two full 16-row bands and a short one: three luma partial sums per image.

Checked here, before anything is written:
  - the numpy model (jitter_model.augment_np) equals Pillow on every case;
  - on the high-saturation image, contrast placed first, in the middle and last sees three different mean lumas m, so a
    reduction taken at the wrong point of the chain changes the result;
  - the half g / half g + 1 grey image has a mean luma of exactly g + 0.5 and Pillow rounds it to m = g + 1.
"""
import itertools
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jitter_model as J  # noqa: E402

OUT = 40
B, C, S = 0, 1, 2
GREY = 117


def jit_row(order, fb, fc, fs):
    bits = np.asarray([fb, fc, fs], dtype=np.float32).view(np.uint32)
    return (len(order),) + tuple(order) + (-1,) * (3 - len(order)) + tuple(int(b) for b in bits)


def main():
    rng = np.random.default_rng(20261019)
    frames = {
        "noise": rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8),
        "noise2": rng.integers(0, 256, size=(48, 60, 3), dtype=np.uint8),
        "const": np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (40, 40, 3)).copy(),
        "binary": (rng.integers(0, 2, size=(64, 64, 3)) * 255).astype(np.uint8),                 # every byte 0 or 255
        "halfgrey": np.repeat(np.where(np.arange(1600).reshape(40, 40) % 2 == 0, GREY, GREY + 1).astype(np.uint8)[:, :, None], 3, 2),
        "vivid": np.stack([rng.integers(170, 256, (40, 40)), rng.integers(0, 60, (40, 40)), rng.integers(0, 256, (40, 40))],
                          -1).astype(np.uint8),                                                  # high saturation, 40 x 40
        "tiny": rng.integers(0, 256, size=(20, 24, 3), dtype=np.uint8),
    }
    names = list(frames)
    offs = dict(zip(names, np.cumsum([0] + [frames[k].size for k in names])[:-1]))
    whole = lambda k: (0, 0) + frames[k].shape[:2]
    orders = list(itertools.permutations((B, C, S)))
    cases = []          # (label, frame, (top, left, h, w), flip, order, (fb, fc, fs))
    for i, o in enumerate(orders):              # all 6 orders: a downscaled crop, and the identity-size high-saturation image
        cases.append((f"order{o}/noise", "noise", (3, 5, 56, 50), i % 2, o, (0.7, 1.6, 0.4)))
        cases.append((f"order{o}/vivid", "vivid", whole("vivid"), (i + 1) % 2, o, (1.3, 0.5, 1.8)))
    cases.append(("empty", "noise", (3, 5, 56, 50), 0, (), (1.0, 1.0, 1.0)))
    cases.append(("empty/flip", "noise2", whole("noise2"), 1, (), (0.3, 0.3, 0.3)))
    for op in (B, C, S):                         # each single operation at factors 0, 1, 2, one in (0, 1), one in (1, 2)
        for i, f in enumerate((0.0, 1.0, 2.0, 0.37, 1.62)):
            fac = [1.0, 1.0, 1.0]
            fac[op] = f
            cases.append((f"single{op}/{f}", "noise2", (2, 4, 44, 52), i % 2, (op,), tuple(fac)))
    for o, fac in (((C, S, B), (2.0, 2.0, 2.0)), ((B, C, S), (0.5, 1.5, 0.0)), ((S, B, C), (1.9, 0.1, 1.1))):
        cases.append((f"const{o}", "const", whole("const"), 0, o, fac))
        cases.append((f"binary{o}", "binary", (0, 0, 64, 64), 1, o, fac))                        # downscale 64 -> 40: overshoot is clipped
    cases.append(("binary/identity", "binary", (7, 11, 40, 40), 0, (S, C, B), (2.0, 2.0, 2.0)))  # pure 0 / 255 into both clip branches
    cases.append(("binary/identity/lo", "binary", (7, 11, 40, 40), 1, (B, S, C), (0.25, 0.75, 0.5)))
    for flip in (0, 1):                          # upscale of a 5 x 7 crop
        cases.append((f"upscale/{flip}", "tiny", (6, 9, 5, 7), flip, (S, C, B), (1.2, 1.7, 0.6)))
    for f in (0.0, 0.5, 1.5):                    # the rounding of m: mean luma exactly GREY + 0.5
        cases.append((f"halfgrey/{f}", "halfgrey", whole("halfgrey"), 0, (C,), (1.0, f, 1.0)))

    desc, jit, res, labels = [], [], [], []
    for label, k, box, flip, order, fac in cases:
        H, W = frames[k].shape[:2]
        t, l, h, w = box
        d = (int(offs[k]), H, W, t, l, h, w, flip, OUT, OUT, 0, 0)
        j = jit_row(order, *fac)
        got = J.augment_pil(frames[k], d, j, OUT, OUT)
        assert np.array_equal(J.augment_np(frames[k], d, j, OUT, OUT), got), label
        desc.append(d), jit.append(j), res.append(got), labels.append(label)

    # contrast first / middle / last on the identity-size vivid image see different means
    v, fac = frames["vivid"], (1.3, 0.5, 1.8)
    m_first = J.contrast_mean(v)
    m_mid = J.contrast_mean(J.enhance(v, B, fac[B]))
    m_last = J.contrast_mean(J.enhance(J.enhance(v, B, fac[B]), S, fac[S]))
    assert len({m_first, m_mid, m_last}) == 3, (m_first, m_mid, m_last)
    assert J.contrast_mean(J.enhance(v, S, fac[S])) != m_first
    # the half-grey image: S / n = GREY + 0.5 exactly, m = GREY + 1 (factor 0 returns the degenerate image itself)
    hg = frames["halfgrey"]
    assert int(J.luma(hg).sum()) * 2 == (2 * GREY + 1) * 1600
    assert np.all(res[labels.index("halfgrey/0.0")] == GREY + 1)
    print("means on vivid (first, middle, last):", m_first, m_mid, m_last)

    out = {"frames": np.concatenate([frames[k].reshape(-1) for k in names]), "desc": np.array(desc, dtype=np.int64),
           "jit": np.array(jit, dtype=np.int64), "out": np.stack(res), "labels": np.array(labels)}
    path = os.path.join(HERE, "m3ae_feed_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
