"""Exactly-summable inputs for the contraction kernels: a test with NO tolerance.

fp32 addition is exact whenever its result is representable.  If every product of a reduction is a multiple of one unit u
and the sum of the products' absolute values stays below 2^24 * u, every partial sum in ANY order, tiling, split-K scheme or
MFMA shape is representable, so a correct kernel returns the mathematically exact result bit for bit -- and so does a plain CPU
fp32 conv2d / matmul, which is the reference.  The bf16 split is exact (x = hi + mid + lo, RNE; csrc/split_common.h), so the
number of significant bits of each operand decides which of the six kept products (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo,
lo*hi) are non-zero, while the three dropped ones (mid*lo, lo*mid, lo*lo) are exactly zero:

  class  operand A                                operand B                                         non-zero products
  D      dense integers, |a| <= 7                 dense integers, |b| <= 7                          hi*hi
  SA     dense multiples of 2^-16, |a| < 4        sparse (<= 8 per reduction), k/2 with |k| <= 3    hi*hi, mid*hi, lo*hi
  SB     A and B of SA swapped                                                                      hi*hi, hi*mid, hi*lo
  SMM    dense multiples of 2^-8, |a| < 4         sparse (<= 16), multiples of 2^-8, |b| < 2        hi*hi, hi*mid, mid*hi, mid*mid

A kernel that loses, doubles or mis-pairs one of these products differs from the reference by hundreds of units.
"""
import math

import torch
import torch.nn.functional as F

CLASSES = ("D", "SA", "SB", "SMM")
SIX = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))          # (plane of A, plane of B), csrc/split_common.h TERM_A / TERM_B
# class -> (kind of A, kind of B, unit of one product)
SPEC = {"D": ("int7", "int7", 1.0), "SA": ("dense18", "half3", 2.0 ** -17), "SB": ("half3", "dense18", 2.0 ** -17),
        "SMM": ("dense10", "sparse9", 2.0 ** -16)}
GRID = {"int7": 1.0, "dense18": 2.0 ** -16, "half3": 0.5, "dense10": 2.0 ** -8, "sparse9": 2.0 ** -8}
NNZ = {"half3": 8, "sparse9": 16}                                 # non-zeros per reduction of the sparse kinds
# the class that proves each product: dropping it from the model must change that class's outputs (test_exact_cpu.py)
PROVES = {(0, 0): "D", (1, 0): "SA", (2, 0): "SA", (0, 1): "SB", (0, 2): "SB", (1, 1): "SMM"}


def unit_of(cls):
    return SPEC[cls][2]


def is_sparse(kind):
    return kind in NNZ


# ---- the CPU model of the arithmetic ---------------------------------------------------------------------------------
def split3(x):
    """x (fp32) -> (hi, mid, lo), each a bf16 value held in fp32, hi + mid + lo == x exactly (RNE three times)."""
    x = x.float()
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def matmul64(a, b):
    return a.double() @ b.double()


def six_term(A, B, drop=None, contract=matmul64, terms=SIX):
    """The kernels' product set in fp64: sum over (i, j) in `terms` (without `drop`) of contract(A_i, B_j)."""
    pa, pb = split3(A), split3(B)
    out = None
    for (i, j) in terms:
        if (i, j) == drop:
            continue
        t = contract(pa[i].double(), pb[j].double())
        out = t if out is None else out + t
    return out


# ---- contractions (any dtype; NHWC activations, HWIO weights like the kernels) ------------------------------------------------
def conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def conv_fwd(x, w, s, p):
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()


def conv_dgrad(dy, w, x_shape, s, p):
    N, H, W, Cin = x_shape
    k = w.shape[0]
    oph = H - ((dy.shape[1] - 1) * s - 2 * p + k)
    opw = W - ((dy.shape[2] - 1) * s - 2 * p + k)
    return F.conv_transpose2d(dy.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=s, padding=p,
                              output_padding=(oph, opw)).permute(0, 2, 3, 1).contiguous()


def conv_wgrad(x, dy, k, s, p):
    """dw (k, k, Cin, Cout): for each tap a (Cin x pixels) @ (pixels x Cout) product over the strided, padded view of x."""
    N, H, W, Cin = x.shape
    OH, OW, Cout = dy.shape[1], dy.shape[2], dy.shape[3]
    xp = F.pad(x, (0, 0, p, p, p, p))
    d2 = dy.reshape(-1, Cout)
    dw = torch.empty((k, k, Cin, Cout), dtype=x.dtype)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s, :].reshape(-1, Cin)
            dw[kh, kw] = xs.t() @ d2
    return dw


# ---- structured positions the sparse operands must contain ------------------------------------------------------------------
def k_positions(K):
    """Reduction indices a K loop goes wrong at: first, last, both sides of every K-stage boundary (16; 32 is among them)."""
    if K <= 256:
        return list(range(K))                                     # short reductions (stem: every tap and channel)
    s = {0, K - 1}
    for b in range(16, K, 16):
        s.update((b - 1, b))
    return sorted(s)


def pixel_positions(N, H, W):
    """Flat pixel indices: first / last pixel of every image, image row, 64- and 256-pixel tile."""
    M = N * H * W
    s = {0, M - 1}
    for n in range(N):
        s.update((n * H * W, (n + 1) * H * W - 1))
    for r in range(N * H):
        s.update((r * W, (r + 1) * W - 1))
    for t in (64, 256):
        for b in range(0, M, t):
            s.update((b, min(b + t, M) - 1))
    return sorted(s)


def _to_rows(shape, axes):
    """Permutation that moves the reduction axes (ascending) behind the others, and the (rows, K) sizes."""
    axes = tuple(sorted(a % len(shape) for a in axes))
    rest = tuple(a for a in range(len(shape)) if a not in axes)
    R = math.prod(shape[a] for a in rest)
    K = math.prod(shape[a] for a in axes)
    return rest + axes, R, K


def forced_mask(shape, sparse_axis, positions, per_row):
    """Boolean mask: row j (an index over the non-reduction axes) holds positions[(j * per_row + t) % P], t < per_row, of its
    reduction (flattened in memory order), so that all rows together cover the whole list when rows * per_row >= P."""
    perm, R, K = _to_rows(shape, sparse_axis)
    pos = torch.as_tensor(positions, dtype=torch.long)
    m = torch.zeros((R, K), dtype=torch.bool)
    j = torch.arange(R * per_row)
    m[j // per_row, pos[j % len(pos)]] = True
    inv = [perm.index(a) for a in range(len(shape))]
    return m.view([shape[a] for a in perm]).permute(inv).contiguous()


def _sparse_mask(shape, count_op, nnz, gen, forced):
    """Random non-zero positions with at most nnz per reduction.  count_op maps the indicator tensor (fp64) to the number of
    non-zeros each reduction sees (a sum over axes, or a convolution of ones for window reductions); elements of over-full
    reductions are thinned at random (never the forced ones) until every reduction fits."""
    longest = count_op(torch.ones(shape, dtype=torch.float64)).max().item()
    m = torch.rand(shape, generator=gen) < min(1.0, 0.9 * nnz / longest)
    if forced is not None:
        m |= forced
    for _ in range(400):
        ind = m.double().requires_grad_(True)
        cnt = count_op(ind)
        over = cnt.detach() > nnz + 0.5
        if not over.any():
            return m
        g, = torch.autograd.grad((cnt * over).sum(), ind)
        bad = (g > 0) & m
        if forced is not None:
            bad &= ~forced
        m = m & ~(bad & (torch.rand(shape, generator=gen) < 0.25))
    raise AssertionError("sparse operand: the forced positions alone exceed the non-zeros allowed per reduction")


def operand(kind, shape, seed, sparse_axis=None, count_op=None, forced=None):
    """One operand of the given kind.  Sparse kinds need sparse_axis (the axes that form the reduction) or count_op."""
    gen = torch.Generator().manual_seed(int(seed))
    shape = tuple(shape)
    ri = lambda lo, hi: torch.randint(lo, hi, shape, generator=gen).double()
    if kind == "int7":
        return ri(-7, 8).float()
    if kind == "dense18":
        return (ri(-(2 ** 18 - 1), 2 ** 18) * 2.0 ** -16).float()
    if kind == "dense10":
        return (ri(-(2 ** 10 - 1), 2 ** 10) * 2.0 ** -8).float()
    if count_op is None:
        axes = tuple(sparse_axis)
        count_op = lambda t: t.sum(dim=axes)
    m = _sparse_mask(shape, count_op, NNZ[kind], gen, forced)
    if kind == "half3":
        v = (ri(1, 4) * (ri(0, 2) * 2 - 1)) * 0.5
    elif kind == "sparse9":
        v = (ri(1, 2 ** 9) * (ri(0, 2) * 2 - 1)) * 2.0 ** -8
    else:
        raise ValueError(kind)
    return (v * m).float()


def pair(cls, shape_a, shape_b, seed, axis_a=None, axis_b=None, count_a=None, count_b=None, forced_a=None, forced_b=None):
    """(A, B, unit) of one class; axis_* / count_* / forced_* describe each operand's reduction for the class where it is the sparse one."""
    ka, kb, unit = SPEC[cls]
    A = operand(ka, shape_a, seed * 2 + 1, axis_a, count_a, forced_a if is_sparse(ka) else None)
    B = operand(kb, shape_b, seed * 2 + 2, axis_b, count_b, forced_b if is_sparse(kb) else None)
    for t, k in ((A, ka), (B, kb)):
        q = t.double() / GRID[k]
        assert torch.equal(q, q.round()), f"class {cls}: operand off its grid"
    return A, B, unit


def window_count(k, s, p):
    """count_op of the input of a convolution: non-zeros per k x k window (all channels), NHWC indicator."""
    def op(t):
        return F.conv2d(t.sum(3)[:, None], torch.ones((1, 1, k, k), dtype=t.dtype), stride=s, padding=p)
    return op


def window_count_t(k, s, p, H, W):
    """count_op of the output gradient of a convolution: non-zeros that reach one input pixel (the transposed convolution)."""
    def op(t):
        one = torch.ones((k, k, 1, 1), dtype=t.dtype)
        return conv_dgrad(t.sum(3, keepdim=True), one, (t.shape[0], H, W, 1), s, p)
    return op


def tap_class_count(s):
    """count_op of the HWIO weights of an input gradient: one output pixel of parity class (py, px) only sees the taps with
    kh = py + pad, kw = px + pad (mod stride), so each (class, input channel) is a reduction of its own over those taps and Cout."""
    def op(t):
        return torch.stack([t[a::s, b::s].sum(dim=(0, 1, 3)) for a in range(s) for b in range(s) if t[a::s, b::s].numel()])
    return op


def window_forced(shape):
    """Forced positions of a window-sparse NHWC operand: first / last pixel of each image and of each 64- / 256-pixel tile, at
    channels on both sides of the K-stage boundaries (rows' ends come with the random positions: the maps are narrow)."""
    N, H, W, C = shape
    M = N * H * W
    s = {0, M - 1}
    for n in range(N):
        s.update((n * H * W, (n + 1) * H * W - 1))
    for b in range(0, M, 64):
        s.update((b, min(b + 64, M) - 1))
    ch = [c % C for c in (0, 15, 16, 31, 32, C - 1)]
    m = torch.zeros((M, C), dtype=torch.bool)
    for i, px in enumerate(sorted(s)):
        m[px, ch[i % len(ch)]] = True
    return m.view(shape)


# ---- the two assertions ---------------------------------------------------------------------------------------------------------
def assert_exact_budget(A, B, unit, contract=matmul64, extra=None, scale=1.0, name="", fp32_bound=False):
    """max(scale * contract(|A|, |B|) + |extra|) < 2^24 * unit, in fp64: every partial sum of every summation order is then an
    exactly representable fp32 value.  `extra`: what an epilogue adds (bias, residual), `scale`: in-place accumulation.
    fp32_bound (the largest cases, where an fp64 convolution costs seconds): the sums of absolute values are formed in fp32 and
    raised by 1 % -- far more than their own rounding error (K * 2^-24 < 0.1 %) -- so the bound is still a bound.
    Returns log2 of the budget used, in units."""
    dt = torch.float32 if fp32_bound else torch.float64
    tot = contract(A.to(dt).abs(), B.to(dt).abs()).double() * scale
    if extra is not None:
        tot = tot + extra.double().abs()
    worst = tot.max().item() / unit * (1.01 if fp32_bound else 1.0)
    assert worst < 2.0 ** 24, f"{name}: sum of |products| = 2^{math.log2(worst):.2f} units: fp32 itself is not exact here"
    return math.log2(max(worst, 1.0))


def sums_are_exact(y, unit):
    """True if the fp64 sums of y and of y^2 over all rows are exact in any order: with y / u integers below 2^24, sum |y| / u is
    far below 2^53, and sum y^2 / u^2 has to be."""
    yi = (y.double() / unit).round().long().reshape(-1, y.shape[-1])
    return yi.abs().max().item() < 2 ** 24 and (yi * yi).sum(0).max().item() < 2 ** 53


def assert_bitwise(got, want, name, unit=None):
    """torch.equal; on failure: how many elements differ, the largest difference in units, the first differing index."""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if got.dtype != want.dtype:
        got, want = got.double(), want.double()
    if torch.equal(got, want):
        return
    d = got.double() - want.double()
    bad = ~(d == 0)                                               # NaN counts as different
    first = torch.nonzero(bad)[0].tolist()
    worst = d[bad].abs().max().item()
    in_units = f" = {worst / unit:.1f} units of {unit:g}" if unit else ""
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; max|d| = {worst:.6e}{in_units}; first at index "
                         f"{first}: got {got[tuple(first)].item()!r}, want {want[tuple(first)].item()!r}")
