"""Restatement of the resident feed's device draw (csrc/resident.hip: resident_draw_kernel) and of its worst-case LDS plan
(csrc/resident_args.h: res_plan) in plain Python: floats are IEEE fp64, `round` is round-half-even as rint is, ints are exact.
tests/test_resident_cpu.py pins the Philox restatement to Random123's known-answer vectors and checks the draw's properties;
tests/test_resident_gpu.py holds the kernel to it row for row."""
import math

M32 = 0xFFFFFFFF
TRIES, FLIP_SLOT = 10, 10
L0 = float.fromhex("-0x1.269621134db92p-2")          # log(3 / 4), the literal of csrc/resident_args.h
L1 = float.fromhex("0x1.269621134db91p-2")           # log(4 / 3)
RATIO_LO, RATIO_HI = 0.75, 4.0 / 3.0

# the dataset and draws of tests/test_resident_gpu.py (that of tests/test_frames_gpu.py::_dataset: clip i has size GPU_SIZES[i % 4])
GPU_SIZES = [(36, 48), (50, 40), (8, 200), (90, 120)]
GPU_N, GPU_T, GPU_SEED, GPU_EPOCHS = 7, 3, 3, (0, 1)


def philox4x32_10(counter, stream_id, seed):
    """Philox4x32-10 of one 64-bit counter: its four 32-bit words (the layout of csrc/philox.h)."""
    c = [counter & M32, counter >> 32, stream_id & M32, stream_id >> 32]
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def block(seed, epoch, index, t, k):
    """key = (epoch << 32) | seed, stream_id = dataset index, counter = (frame slot << 4) | k."""
    assert 0 <= seed < 1 << 32 and 0 <= epoch < 1 << 32
    return philox4x32_10((t << 4) | k, index, (epoch << 32) | seed)


def fallback(H, W):
    """The central crop of frames.sample_crop after ten refused tries."""
    in_ratio = float(W) / float(H)
    w, h = W, H
    if in_ratio < RATIO_LO:
        h = int(round(W / RATIO_LO))
    elif in_ratio > RATIO_HI:
        w = int(round(H * RATIO_HI))
    return (H - h) // 2, (W - w) // 2, h, w


def draw(H, W, seed, epoch, index, t):
    """((top, left, h, w, flip), tries made, accepted, margin): margin is the least distance of any evaluated root from a
    half-integer, over every try made."""
    area = float(H * W)
    box, tries, margin = None, 0, 0.5
    for k in range(TRIES):
        a, b, c, d = block(seed, epoch, index, t, k)
        tries += 1
        u, v = a * 2.0 ** -32, b * 2.0 ** -32
        target = area * (0.08 + 0.92 * u)
        aspect = math.exp(L0 + (L1 - L0) * v)
        rw, rh = math.sqrt(target * aspect), math.sqrt(target / aspect)
        margin = min(margin, abs(rw - math.floor(rw) - 0.5), abs(rh - math.floor(rh) - 0.5))
        w, h = int(round(rw)), int(round(rh))
        if 0 < w <= W and 0 < h <= H:
            box = ((c * (H - h + 1)) >> 32, (d * (W - w + 1)) >> 32, h, w)
            break
    accepted = box is not None
    if not accepted:
        box = fallback(H, W)
    flip = int(block(seed, epoch, index, t, FLIP_SLOT)[0] < 1 << 31)
    return box + (flip,), tries, accepted, margin


def desc_row(offset, H, W, seed, epoch, index, t, train=True):
    """The 8-column descriptor row the draw kernel writes."""
    if not train:
        return (offset, H, W, 0, 0, H, W, 0)
    return (offset, H, W) + draw(H, W, seed, epoch, index, t)[0]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
FR_BAND, FR_LDS_MAX = 16, 65536


def bounds(n_in, n_out, xx):
    """Pillow precompute_coeffs (bilinear): first source index and count of output index xx."""
    scale = n_in / n_out
    support = 1.0 * max(scale, 1.0)
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), n_in)
    return xmin, xmax - xmin


def ksize(n_in, n_out):
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def _al(b):
    return (b + 15) & ~15


def lds_bytes(OW, band, rows_cap, kh, kv):
    return _al(3 * 256 * 4) + _al(OW * kh * 4) + _al(OW * 8) + _al(band * kv * 4) + _al(band * 8) + _al(rows_cap * OW * 3)


def band_rows(ch, OH, band):
    rows = 1
    for y0 in range(0, OH, band):
        a0, _ = bounds(ch, OH, y0)
        b0, b1 = bounds(ch, OH, min(y0 + band, OH) - 1)
        rows = max(rows, b0 + b1 - a0)
    return rows


def plan(shapes, OH, OW, train):
    """(band, rows_cap, kh, kv, lds) over every crop height 1..H and width 1..W of every shape (train), or the whole frames."""
    kh = max(ksize(W, OW) for _, W in shapes)
    kv = max(ksize(H, OH) for H, _ in shapes)
    band = FR_BAND
    while band >= 1:
        heights = range(1, max(H for H, _ in shapes) + 1) if train else sorted({H for H, _ in shapes})
        rows_cap = max(band_rows(ch, OH, band) for ch in heights)
        lds = lds_bytes(OW, band, rows_cap, kh, kv)
        if lds <= FR_LDS_MAX:
            return band, rows_cap, kh, kv, lds
        band >>= 1
    return None
