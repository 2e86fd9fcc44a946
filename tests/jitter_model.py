"""The M3AE train image transform restated in numpy (no GPU, no PIL needed) and, beside it, the same through PIL itself.

Pillow's ImageEnhance.Brightness / Contrast / Color are Image.blend(degenerate, image, factor) (libImaging/Blend.c):
    per byte, fp32, product and sum rounded separately:  t = (float)d + a * (float)((int)x - (int)d)
    0 <= a <= 1: (uint8)t;  otherwise 0 if t <= 0, 255 if t >= 255, else (uint8)t
    brightness  d = 0
    saturation  d = L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 of the pixel (ImagingConvert rgb2l), in all channels
    contrast    d = m = int(S / n + 0.5), S = the sum of L over the image as it is when contrast is applied
Operation ids are torchvision ColorJitter's fn_id: 0 brightness, 1 contrast, 2 saturation.  Crop, bicubic resize and flip come from
the numpy / PIL models of test_cav_feed_cpu.py.
"""
import numpy as np

from test_cav_feed_cpu import pil_window, resample_np

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2


def blend(d, x, a):
    """d, x uint8 arrays (broadcastable), a a Python float or np.float32 -> uint8."""
    a = np.float32(a)
    diff = (x.astype(np.int32) - d.astype(np.int32)).astype(np.float32)
    t = d.astype(np.float32) + a * diff                     # two fp32 roundings: numpy does not contract
    assert t.dtype == np.float32
    if np.float32(0) <= a <= np.float32(1):
        return t.astype(np.uint8)                            # t lies between d and x: plain truncation
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def luma(img):
    """uint8 (H, W, 3) -> int64 (H, W): PIL's RGB -> L."""
    p = img.astype(np.int64)
    return (p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16


def contrast_mean(img):
    """int(S / n + 0.5) with a double division; the integer form (2 S + n) // (2 n) is asserted equal."""
    L = luma(img)
    S, n = int(L.sum()), L.size
    m = int(S / n + 0.5)
    assert m == (2 * S + n) // (2 * n)
    return m


def enhance(img, op, a):
    if op == BRIGHTNESS:
        d = np.zeros_like(img)
    elif op == CONTRAST:
        d = np.full_like(img, contrast_mean(img))
    elif op == SATURATION:
        d = np.repeat(luma(img).astype(np.uint8)[..., None], 3, axis=2)
    else:
        raise ValueError(op)
    return blend(d, img, a)


def jitter_np(img, order, factors):
    """order: operation ids as applied; factors: (brightness, contrast, saturation)."""
    for op in order:
        img = enhance(img, op, factors[op])
    return img


def unpack_jitter(row):
    """A jitter descriptor row -> (order, fp32 factors)."""
    n = int(row[0])
    order = tuple(int(v) for v in row[1:1 + n])
    factors = tuple(float(f) for f in np.asarray(row[4:7], dtype=np.int64).astype(np.uint32).view(np.float32))
    return order, factors


def augment_np(frame, desc_row, jit_row, OH, OW):
    """uint8 (OH, OW, 3): crop -> bicubic resize (+ window) -> flip -> jitter, all numpy."""
    return jitter_np(resample_np(frame, *[int(v) for v in desc_row[3:12]], OH, OW), *unpack_jitter(jit_row))


def jitter_pil(img, order, factors):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(img))
    cls = {BRIGHTNESS: ImageEnhance.Brightness, CONTRAST: ImageEnhance.Contrast, SATURATION: ImageEnhance.Color}
    for op in order:
        im = cls[op](im).enhance(factors[op])
    return np.asarray(im)


def augment_pil(frame, desc_row, jit_row, OH, OW):
    """The same with Pillow's own resize and ImageEnhance."""
    return jitter_pil(pil_window(frame, *[int(v) for v in desc_row[3:12]], OH, OW), *unpack_jitter(jit_row))
