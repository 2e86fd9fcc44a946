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
import functools
import math
from types import SimpleNamespace

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


# ==================================================================================================================================
# Exactly-summable inputs for the REDUCTIONS between the contractions: BatchNorm statistics and backward sums with their finalize
# paths, the reductions fused into the input-gradient epilogue and the pooled stem backward, column sums, LayerNorm affine gradients
# (test_reduce_exact_cpu.py proves the builders, test_reduce_exact_gpu.py runs the kernels).
#
# All data are small integers held in fp32, scaled where needed by a power of two: mean is an integer per channel (per row for
# LayerNorm), invstd / rstd a power of two, gamma +-2^j, beta an integer.  Then x * x, g * ((x - mean) * invstd) and bn(x) are exact
# in fp32, contracted to an fma or not, every term of a sum is a multiple of one unit, and with  sum |term| < 2^24 units  per output
# (assert_sum_budget, checked before anything is launched) every partial sum in any order, tiling or finalize path is exact.  The
# reference is int64 arithmetic; a lost, doubled or mis-paired row or tile is off by whole units.
# ==================================================================================================================================
SUM_BUDGET = 2 ** 24
G_UNIT = 2.0 ** -3            # upstream gradients are integers / 8: |g| < 1, see bn_rows_case on the dx tolerance
BN_EPS32 = torch.tensor(1e-5, dtype=torch.float32).double().item()          # the kernels take eps and momentum as fp32
BN_MOM32 = torch.tensor(0.1, dtype=torch.float32).double().item()


def rand_ints(shape, lo, hi, seed, nonzero=False, dtype=torch.int64):
    """Uniform integers in [lo, hi]; nonzero: in [lo, -1] and [1, hi] (lo < 0 < hi)."""
    g = torch.Generator().manual_seed(int(seed))
    if not nonzero:
        return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=dtype)
    r = torch.randint(lo, hi, tuple(shape), generator=g, dtype=dtype)
    return r + (r >= 0).to(dtype)


def assert_sum_budget(abs_units, name=""):
    """abs_units: per output element the sum over ALL rows (tiles) of |term| / unit, as integers.  Below 2^24 every partial sum of
    every summation order is an exactly representable fp32 value (and an fp64 one by a wide margin).  Returns log2 of the budget used."""
    worst = int(torch.as_tensor(abs_units).max())
    assert worst < SUM_BUDGET, f"{name}: sum of |terms| = 2^{math.log2(max(worst, 1)):.2f} units: fp32 partial sums are not exact here"
    return math.log2(max(worst, 1))


def exact_f32(units, unit):
    """int64 units * unit (a power of two, scalar or per element) as fp32; nothing may round on the way."""
    d = units.double() * unit
    f = d.float()
    assert torch.equal(f.double(), d), "an exact total is not representable in fp32"
    return f


def bn_channels(C, seed):
    """Per-channel BatchNorm parameters on which xhat and bn(x) are exact for integer x: integer mean and beta, invstd = 2^-k with
    k in 1..3 (so xhat of x = mean +- 8 is of unit scale, like real normalised data), gamma = +-2^j with j in -1..1; |gamma * invstd| <= 1."""
    mean_i, k = rand_ints((C,), -3, 3, seed), rand_ints((C,), 1, 3, seed + 1)
    sign, j = rand_ints((C,), 0, 1, seed + 2) * 2 - 1, rand_ints((C,), -1, 1, seed + 3)
    return SimpleNamespace(C=C, mean_i=mean_i, k=k, mean=mean_i.float(), invstd=(2.0 ** -k.double()).float(),
                           gamma=(sign.double() * 2.0 ** j.double()).float(), beta=rand_ints((C,), -2, 2, seed + 4).float())


# ---- 1. finalize regimes: fabricated per-tile partials ------------------------------------------------------------------------------
FINALIZE_TILES = (1, 15, 16, 17, 63, 64, 65,            # lanes unused / one trip / tail of the one-launch kernel
                  1023, 1024, 1025,                     # one-launch | wide boundary
                  1025 + 191, 1025 + 256,               # wide kernel: unrolled trip present / absent
                  16383, 16384, 16385, 20001, 40000)    # wide | two-stage boundary; ragged last chunk
FINALIZE_CASES = [(C, t) for C in (4, 64) for t in FINALIZE_TILES] + [(1024, t) for t in FINALIZE_TILES if t <= 1025]


def _separate_slots(p):
    """Make the totals of slot 0 and slot 1 differ in every channel (a kernel that swaps the slots must be seen everywhere): where
    they are equal the sign of slot 1's first tile is flipped, which moves that total by 2 |v| != 0 and keeps sum |v|."""
    same = p[:, 0].sum(0) == p[:, 1].sum(0)
    p[0, 1] = torch.where(same, -p[0, 1], p[0, 1])
    return p


def bwd_partials(tiles, C, seed):
    """fp32 [tiles][2][C] per-tile (sum g, sum g * xhat) rows as bn_reduce_kernel<1> writes them: non-zero integers, so a dropped or
    doubled tile moves a total by at least 1; tiles * max|v| < 2^20: with a power-of-two row count in the apply pass that follows, dgamma / M, dbeta / M and xhat * dgamma / M are then exact too."""
    amax = min(1000, (2 ** 20 - 1) // tiles)
    p = _separate_slots(rand_ints((tiles, 2, C), -amax, amax, seed, nonzero=True))
    assert (p != 0).all() and (tiles == 1 or (p.min(0).values != p.max(0).values).all()), "tile contributions must be non-zero and distinct"
    assert_sum_budget(p.abs().sum(0), f"backward partials, {tiles} tiles")
    tot = p.sum(0)
    assert (tot[0] != tot[1]).all()
    return SimpleNamespace(tiles=tiles, C=C, ints=p, partial=p.float(), dbeta=exact_f32(tot[0], 1.0), dgamma=exact_f32(tot[1], 1.0))


def fwd_rows(tiles):
    """The row count M = 2^k the forward cases pair with `tiles` tiles: about 32 to 64 rows per tile."""
    return 1 << (32 * tiles - 1).bit_length()


def fwd_partials(tiles, C, seed):
    """fp64 [tiles][2][C] per-tile (sum x, sum x^2) rows as the conv epilogue / bn_reduce_kernel<0> write them, for M = 2^k rows (about
    32 to 64 per tile): sum x in [-32, 96] without 0, sum x^2 in [1024, 4095].  Then |mean| <= 3 and E[x^2] > 16, so the variance is
    above 7 -- far from the cancellation of E[x^2] - E[x]^2 -- and s / M is exact in fp64 AND in fp32 (s < 2^24).
    The running mean starts at multiples of 1/4: (1 - momentum) * rm + momentum * mean is then exact in fp64 whether the compiler
    contracts it or not (running_units), so after the one rounding to fp32 the kernel's value must equal the reference bit for bit."""
    M = fwd_rows(tiles)
    s = rand_ints((tiles, 1, C), -32, 96, seed, nonzero=True)
    q = rand_ints((tiles, 1, C), 1024, 4095, seed + 1)
    p = torch.cat([s, q], 1)
    assert_sum_budget(s.abs().sum(0), f"forward partials, {tiles} tiles")
    assert int(q.sum(0).max()) < 2 ** 53
    rm4 = rand_ints((C,), -8, 8, seed + 2)
    rv = (rand_ints((C,), 2, 12, seed + 3).double() / 4).float()
    return SimpleNamespace(tiles=tiles, C=C, M=M, ints=p, partial=p.double(), S=p[:, 0].sum(0), Q=p[:, 1].sum(0), rm4=rm4,
                           running_mean=(rm4.double() / 4).float(), running_var=rv)


def bn_stats_ref(S, Q, M, running_mean=None, running_var=None):
    """The statistics of mla_bn_finalize in fp64, from the exact integer totals: mean, invstd[, running_mean, running_var]."""
    m = S.double() / M
    var = (Q.double() / M - m * m).clamp_min(0.0)
    out = [m, 1.0 / torch.sqrt(var + BN_EPS32)]
    if running_mean is not None:
        unb = var * (float(M) / float(max(M - 1, 1)))
        out += [(1.0 - BN_MOM32) * running_mean.double() + BN_MOM32 * m, (1.0 - BN_MOM32) * running_var.double() + BN_MOM32 * unb]
    return out


def running_units(S, rm4, M):
    """(1 - momentum) * rm4 / 4 + momentum * S / M as an integer count of 2^-29 / M (M = 2^k): momentum = a / 2^27 exactly (fp32 0.1),
    so the value is ((2^27 - a) * rm4 * M + 4 * a * S) units, below 2^53: every fp64 evaluation of it is exact."""
    a = int(BN_MOM32 * 2 ** 27)
    assert a / 2 ** 27 == BN_MOM32 and M & (M - 1) == 0
    u = (2 ** 27 - a) * rm4 * M + 4 * a * S
    assert int(u.abs().max()) < 2 ** 53
    return u, 2.0 ** -29 / M


# ---- 1b. the ORDER in which each finalize regime adds the tiles of one channel ---------------------------------------------------------
# On the integer data above every order gives the same bits, so those cases cannot see a change of the fp64 summation order -- which
# decides the last bit of every mean, dgamma and dbeta in training.  Here the order of csrc/bn.hip is restated in torch fp64 (IEEE
# addition, like the device's v_add_f64: no fast-math on either side) and run on CANCELLING partials, whose channel total is rounding
# residue and nothing else.  p is [tiles][...] (any trailing shape: slots and channels are carried along), widened to fp64 first.
BN_ONE_MAXT, BN_WIDE_MAXT = 1024, 16384          # the regime thresholds of csrc/bn.hip
ORDER_REGIMES = ("narrow", "wide", "two_stage")


def finalize_regime(tiles):
    return "narrow" if tiles <= BN_ONE_MAXT else "wide" if tiles <= BN_WIDE_MAXT else "two_stage"


def lane_order_total(p, KL):
    """bn_finalize_tiles_kernel with KL tile lanes (narrow: 16, wide: 64).  Lane k starts at tile k; while t + 3 KL < tiles it adds
    (p[t] + p[t+KL]) + (p[t+2KL] + p[t+3KL]) and steps 4 KL, then it adds p[t] singly in steps of KL; lane 0 adds lanes 1..KL-1 in
    ascending order.  One loop trip here is one block of 4 KL tiles: the first `full` lanes take the unrolled form, the others are
    in their tail (a lane that left the unrolled loop never re-enters it, and its tail ends inside the same block)."""
    p = p.double()
    tiles = p.shape[0]
    s = torch.zeros((KL,) + p.shape[1:], dtype=torch.float64)
    for t in range(0, tiles, 4 * KL):
        full = min(max(tiles - t - 3 * KL, 0), KL)
        if full:
            a = [p[t + j * KL:t + j * KL + full] for j in range(4)]
            s[:full] += (a[0] + a[1]) + (a[2] + a[3])
        for j in range(4):
            lo, hi = t + j * KL + full, min(t + (j + 1) * KL, tiles)
            if lo < hi:
                s[full:full + hi - lo] += p[lo:hi]
    tot = s[0].clone()
    for k in range(1, KL):
        tot += s[k]
    return tot


def two_stage_order_total(p):
    """bn_tiles_stage1_kernel + chunk_sums.  S = clamp(cdiv(tiles, 64), 1, 64) chunks of per = cdiv(tiles, S) tiles; in a chunk wave w
    of 4 adds tiles t0 + w, t0 + w + 4, ... one by one, wave 0 then adds waves 1..3; stage 2: lane kl of 4 adds the chunk sums kl,
    kl + 4, ... in ascending order (absent chunks count as 0.0), lane 0 then adds lanes 1..3.  Tiles past the end of a chunk are
    zero-padded here: a running sum that starts at +0.0 is never -0.0, so adding +0.0 leaves its bits alone."""
    p = p.double()
    tiles, rest = p.shape[0], p.shape[1:]
    S = min(max(-(-tiles // 64), 1), 64)
    per = -(-tiles // S)
    trips = -(-per // 4)
    pad = torch.zeros((S, trips * 4) + rest, dtype=torch.float64)
    for y in range(S):
        n = max(min(tiles, (y + 1) * per) - y * per, 0)
        pad[y, :n] = p[y * per:y * per + n]
    pad = pad.view((S, trips, 4) + rest)
    w = torch.zeros((S, 4) + rest, dtype=torch.float64)
    for i in range(trips):
        w += pad[:, i]
    chunk = torch.zeros((64,) + rest, dtype=torch.float64)
    chunk[:S] = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    chunk = chunk.view((16, 4) + rest)
    lane = torch.zeros((4,) + rest, dtype=torch.float64)
    for j in range(16):
        lane += chunk[j]
    return ((lane[0] + lane[1]) + lane[2]) + lane[3]


def sequential_total(p):
    """Plain tile-by-tile fp64 sum (no kernel's order: what the cancelling tile is built from, and a fourth order to tell apart)."""
    p = p.double()
    tot = torch.zeros(p.shape[1:], dtype=torch.float64)
    for t in range(p.shape[0]):
        tot += p[t]
    return tot


def order_total(p, regime=None):
    """The fp64 total of every channel of p, added in the order of `regime` (default: the regime this tile count lands in)."""
    regime = regime or finalize_regime(p.shape[0])
    return lane_order_total(p, 16) if regime == "narrow" else lane_order_total(p, 64) if regime == "wide" else two_stage_order_total(p)


def _cancel_tail(p, n_split):
    """Replace the last min(n_split, tiles - 1) tiles of p by minus the sequential fp64 sum of the tiles before them, split into
    that many values of p's dtype (the value itself last, before it what its rounding left, ...).  One fp64 value, or three fp32 values (72 >= 53
    bits), hold that sum exactly, so the mathematical total of every channel is zero.  A single tile stays as drawn."""
    k = min(n_split, p.shape[0] - 1)
    if k:
        r = -sequential_total(p[:-k])
        for i in range(1, k + 1):                # the leading part goes last: the closing tile is never a zero
            p[-i] = r.to(p.dtype)
            r = r - p[-i].double()
        assert (r == 0).all(), "the split must hold the sum exactly"
    return p


def cancelling_partials(tiles, C, seed):
    """[tiles][2][C] partial rows whose channel totals are pure rounding residue: non-integers with a wide exponent spread,
    randn * 2^randint(-20, 20) per element, closed by tiles that cancel the sequential fp64 sum of the others (_cancel_tail).
    The bits of a total then depend on the order of the additions and on nothing else.  `fwd`: fp64, as the forward statistics
    arrive; `bwd`: generated in fp32 (a product of an fp32 value and a power of two), so that the kernel's widening is exact --
    there the sum of the others needs three fp32 tiles to cancel to the last fp64 bit: with one, its fp32 rounding (2^-24 of
    the sum) would bury the order's residue (2^-53) beyond what an fp32 result resolves."""
    g = torch.Generator().manual_seed(int(seed) + 1)     # (+ 1: with + 0 the case 1216 x 4 misses test_cancelling_partials_tell_orders_apart)

    def draw(dtype):
        v = torch.randn((tiles, 2, C), generator=g, dtype=dtype)
        return v * (2.0 ** torch.randint(-20, 21, (tiles, 2, C), generator=g).double()).to(dtype)
    return SimpleNamespace(tiles=tiles, C=C, M=fwd_rows(tiles), fwd=_cancel_tail(draw(torch.float64), 1), bwd=_cancel_tail(draw(torch.float32), 3))


# ---- 2. producer kernels over [M][C] rows -------------------------------------------------------------------------------------------
BN_C = (4, 8, 16, 32, 64, 256, 1024)
BN_WRAP_N4 = 8192 * 256 + 448          # float4 elements: the elementwise grid is capped at 8192 workgroups of 256 threads


def bn_row_counts(C):
    """M = 1, 3, one either side of the number of row lanes (1024 / C) and of the 32-row tile, two tiles + 1; for C = 4 and 64 also
    65537, 2^18 + 1 (the tile rule changes, more than 1024 tiles) and the first M whose elementwise pass wraps its grid-stride loop."""
    nrl = 1024 // C
    ms = {1, 3, nrl - 1, nrl + 1, 31, 32, 33, 2 * 32 + 1}
    if C in (4, 64):
        ms |= {65537, 2 ** 18 + 1, BN_WRAP_N4 * 4 // C}
    return sorted(m for m in ms if m > 0)


BN_ROW_CASES = [(M, C) for C in BN_C for M in bn_row_counts(C)]


def bn_rows_case(M, C, seed):
    """x = mean + d with integer |d| <= D, g = integer / 8 with |integer| <= G, an integer residual; (G, D) shrinks with M so that
    M * G * D < 2^24.  Terms of sum g are multiples of 1/8, terms of sum g * xhat multiples of invstd / 8.

    Why g is scaled by 1/8: the apply passes are held to the fp64 formula at atol 1e-6, rtol 2e-5.  With r = g - a - b, a = dbeta / M,
    b = xhat * dgamma / M, every fp32 rounding of the kernel is relative to one of the terms (< 3e-7 in all).  |g|, |a| < 1, so either
    |b| >= 2, then |r| >= |b| / 8 and the relative error of r is below 3e-6, or |b| < 2 and the absolute error is below 1e-6;
    |gamma * invstd| <= 1 scales both alike.  Cancellation cannot push a correct kernel over the tolerance."""
    G, D = next((g, d) for g, d in ((7, 8), (3, 5), (2, 3), (1, 3)) if M * g * d < SUM_BUDGET)
    ch = bn_channels(C, seed)
    i32 = torch.int32
    dev, gi = rand_ints((M, C), -D, D, seed + 10, dtype=i32), rand_ints((M, C), -G, G, seed + 11, dtype=i32)
    ri = rand_ints((M, C), -3, 3, seed + 12, dtype=i32)
    assert_sum_budget(gi.abs().sum(0, dtype=torch.int64), f"sum g, M={M} C={C}")
    assert_sum_budget((gi * dev).abs().sum(0, dtype=torch.int64), f"sum g * xhat, M={M} C={C}")
    xi = dev + ch.mean_i.to(i32)
    assert int((xi.long() * xi.long()).sum(0).max()) < 2 ** 53
    return SimpleNamespace(M=M, C=C, ch=ch, dev=dev, gi=gi, xi=xi, x=xi.float(), g=(gi.double() * G_UNIT).float(), res=ri.float())


def bn_stat_sums(case):
    """(sum x, sum x^2) per channel, int64."""
    xl = case.xi.long()
    return xl.sum(0), (xl * xl).sum(0)


def bn_bwd_sums(case, mask=None):
    """Exact (dgamma, dbeta) as fp32; mask (bool [M][C]): the rows the ReLU passes."""
    gi = case.gi if mask is None else case.gi * mask.to(case.gi.dtype)
    db, dg = gi.sum(0, dtype=torch.int64), (gi * case.dev).sum(0, dtype=torch.int64)
    return exact_f32(dg, G_UNIT * case.ch.invstd.double()), exact_f32(db, G_UNIT)


def bn_apply_rows(x, ch, relu=False, residual=None):
    """relu(bn(x) + residual) in fp64 (exact on these inputs)."""
    y = ((x.double() - ch.mean.double()) * ch.invstd.double()) * ch.gamma.double() + ch.beta.double()
    if residual is not None:
        y = y + residual.double()
    return y.clamp_min(0.0) if relu else y


def bn_dx_rows(g, x, ch, dgamma, dbeta, M):
    """The BatchNorm input gradient in fp64 from given dgamma / dbeta: gamma * invstd * (g - dbeta / M - xhat * dgamma / M)."""
    xhat = (x.double() - ch.mean.double()) * ch.invstd.double()
    return ch.gamma.double() * ch.invstd.double() * (g.double() - dbeta.double() / M - xhat * (dgamma.double() / M))


# ---- 3a. BatchNorm-backward reductions in the input-gradient epilogue ---------------------------------------------------------------
DGRAD_BN_GEOMS = [      # (N, H, W, Cin, Cout, k, s, p), conv2d_patch setting (None: leave the planner's)
    ((2, 9, 7, 64, 128, 3, 2, 1), None),
    ((2, 33, 17, 128, 128, 3, 1, 1), None),
    ((2, 20, 12, 64, 128, 3, 2, 1), None),      # a merged stride-2 geometry (the four parity classes in one launch)
    ((2, 56, 56, 64, 64, 3, 1, 1), 2),          # the LDS-patch kernels' epilogues (persistent 64 -> 64 and one tile per workgroup)
]


def dgrad_bn_case(geom, seed):
    """Class D operands (integer dy, w and residual, |.| <= a): dx is an exact integer map.  Two BatchNorm requests with integer inputs
    z_q = mean_q + d_q, |d_q| <= D.  (a, D) shrink until  sum (|dx| + |residual|) * |d_q| < 2^24  per channel, which bounds the terms of
    every operand combination (with / without residual, ReLU mask)."""
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = conv_out(H, k, s, p), conv_out(W, k, s, p)
    con = lambda a, b: conv_dgrad(a, b, (N, H, W, Cin), s, p)
    chs = [bn_channels(Cin, seed + 20 + 10 * q) for q in range(2)]
    for a, D in ((7, 8), (5, 8), (3, 8), (3, 4), (2, 4), (2, 2), (1, 2), (1, 1)):
        dy, w = rand_ints((N, OH, OW, Cout), -a, a, seed).float(), rand_ints((k, k, Cin, Cout), -a, a, seed + 1).float()
        res = rand_ints((N, H, W, Cin), -a, a, seed + 2)
        assert_exact_budget(dy, w, 1.0, contract=con, name=f"dgrad {geom}")
        dx = con(dy, w)
        devs = [rand_ints((N, H, W, Cin), -D, D, seed + 3 + q) for q in range(2)]
        bound = dx.long().abs() + res.abs()
        if max(int((bound * d.abs()).reshape(-1, Cin).sum(0).max()) for d in devs) < SUM_BUDGET:
            break
    for d in devs:
        assert_sum_budget((bound * d.abs()).reshape(-1, Cin).sum(0), f"dgrad epilogue sum v * xhat {geom}")
    assert_sum_budget(bound.reshape(-1, Cin).sum(0), f"dgrad epilogue sum v {geom}")
    msk = torch.randn((N, H, W, Cin), generator=torch.Generator().manual_seed(seed + 5))
    return SimpleNamespace(geom=geom, dy=dy, w=w, res=res.float(), msk=msk, dx=dx, chs=chs, devs=devs, amax=a,
                           zs=[(d + c.mean_i).float() for d, c in zip(devs, chs)])


def dgrad_bn_sums(case, v, q):
    """Exact (dgamma_q, dbeta) of the stored map v (integers in fp32) for request q."""
    C = v.shape[-1]
    vi = v.long().reshape(-1, C)
    assert torch.equal(vi.float(), v.reshape(-1, C))
    return exact_f32((vi * case.devs[q].reshape(-1, C)).sum(0), case.chs[q].invstd.double()), exact_f32(vi.sum(0), 1.0)


# ---- 3b. the pooled stem backward -----------------------------------------------------------------------------------------------------
POOLED_CASES = [(1, 2, 2, 64), (3, 9, 7, 64), (2, 16, 12, 64), (8, 112, 40, 64)]      # the last one: more than one tile of pooled rows


def pooled_case(N, H, W, C, seed):
    """y = mean + d (|d| <= 8) and an integer pooled gradient (|.| <= 7, non-zero): bn(y), the ReLU mask and xhat are exact."""
    ch = bn_channels(C, seed)
    OH, OW = conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1)
    dev = rand_ints((N, H, W, C), -8, 8, seed + 10)
    dpool = rand_ints((N, OH, OW, C), -7, 7, seed + 11, nonzero=True)
    assert_sum_budget(torch.tensor(N * OH * OW * 7 * 8), f"pooled sums {N}x{H}x{W}")       # whatever the max-pool selects
    y = (dev + ch.mean_i).float()
    return SimpleNamespace(N=N, H=H, W=W, C=C, OH=OH, OW=OW, ch=ch, dev=dev, dpool_i=dpool, dpool=dpool.float(), y=y, act=bn_apply_rows(y, ch, relu=True))


def pooled_idx_cpu(case):
    """The max-pool decisions on the CPU (first maximum in row-major window order), as codes kh * 3 + kw like the kernels'."""
    _, flat = F.max_pool2d(case.act.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    flat = flat.permute(0, 2, 3, 1)
    oy, ox = torch.arange(case.OH).view(1, -1, 1, 1), torch.arange(case.OW).view(1, 1, -1, 1)
    return ((flat // case.W - (oy * 2 - 1)) * 3 + (flat % case.W - (ox * 2 - 1))).to(torch.uint8)


def pooled_sums(case, idx):
    """Exact scatter-form sums over the POOLED outputs o: dbeta = sum dpool[o] [bn(y[sel o]) > 0], dgamma likewise with xhat(y[sel o]).
    Returns (dgamma, dbeta, selected values of relu(bn(y)))."""
    code = idx.long()
    assert int(code.max()) <= 8
    oy, ox = torch.arange(case.OH).view(1, -1, 1, 1), torch.arange(case.OW).view(1, 1, -1, 1)
    iy, ix = oy * 2 - 1 + code // 3, ox * 2 - 1 + code % 3
    assert int(iy.min()) >= 0 and int(iy.max()) < case.H and int(ix.min()) >= 0 and int(ix.max()) < case.W, "a selected pixel lies in the padding"
    flat = (iy * case.W + ix).reshape(case.N, -1, case.C)
    d_sel = case.dev.reshape(case.N, -1, case.C).gather(1, flat)
    a_sel = case.act.reshape(case.N, -1, case.C).gather(1, flat)
    gm = case.dpool_i.reshape(case.N, -1, case.C) * (a_sel > 0)
    return exact_f32((gm * d_sel).sum((0, 1)), case.ch.invstd.double()), exact_f32(gm.sum((0, 1)), 1.0), a_sel.reshape(case.N, case.OH, case.OW, case.C)


def pooled_gather(case, idx):
    """The same upstream gradient in gather form, fp64 [N][H][W][C]: the pooled gradient scattered to the selected pixels (a pixel may be
    selected by up to four windows), times the ReLU mask."""
    code = idx.long()
    oy, ox = torch.arange(case.OH).view(1, -1, 1, 1), torch.arange(case.OW).view(1, 1, -1, 1)
    flat = ((oy * 2 - 1 + code // 3) * case.W + (ox * 2 - 1 + code % 3)).reshape(case.N, -1, case.C)
    g = torch.zeros((case.N, case.H * case.W, case.C), dtype=torch.float64).scatter_add_(1, flat, case.dpool.double().reshape(case.N, -1, case.C))
    return (g * (case.act.reshape(case.N, -1, case.C) > 0)).reshape(case.N, case.H, case.W, case.C)


# ---- 4. transformer column reductions -----------------------------------------------------------------------------------------------
COLSUM_CASES = [(M, C) for C in (64, 768, 1024) for M in (1, 15, 16, 17, 63, 64, 65, 4097, 16385 + 3)]
LN_CASES = [(M, D) for D in (512, 768, 1024) for M in (1, 3, 15, 16, 17, 1025, 4099)]     # 1025 rows: more than 64 row blocks of 16


def colsum_case(M, C, seed):
    xi = rand_ints((M, C), -7, 7, seed)
    assert_sum_budget(xi.abs().sum(0), f"column sums {M}x{C}")
    return SimpleNamespace(x=xi.float(), total=exact_f32(xi.sum(0), 1.0), xi=xi)


def ln_case(M, D, seed):
    """LayerNorm backward: x = mean[row] + d (|d| <= 8), rstd[row] = 2^-k, k in 1..3, dy and add = integers / 8, w = +-2^j per column.
    db sums multiples of 1/8, dw multiples of 2^-6 (dy * d * 2^-k).  dx (atol 1e-5, rtol 1e-5): r = g - mean(g) - b, b = xhat * mean(g * xhat),
    |g| = |dy * w| < 2, and the fp32 roundings are below 3e-7 relative to a term.  Either |b| >= 8, then |r| >= |b| / 2 and the relative
    error is below 1e-6, or |b| < 8 and the absolute error is below 4e-6; rstd <= 1/2 scales both alike."""
    mean_i, k = rand_ints((M, 1), -3, 3, seed), rand_ints((M, 1), 1, 3, seed + 1)
    dev, dyi = rand_ints((M, D), -8, 8, seed + 2), rand_ints((M, D), -7, 7, seed + 3)
    sign, j = rand_ints((D,), 0, 1, seed + 4) * 2 - 1, rand_ints((D,), -1, 1, seed + 5)
    addi = rand_ints((M, D), -7, 7, seed + 6)
    dw_units = dyi * dev * 2 ** (3 - k)                                          # units of 2^-6
    assert_sum_budget(dyi.abs().sum(0), f"LayerNorm db {M}x{D}")
    assert_sum_budget(dw_units.abs().sum(0), f"LayerNorm dw {M}x{D}")
    return SimpleNamespace(M=M, D=D, x=(dev + mean_i).float(), dy=(dyi.double() * G_UNIT).float(), add=(addi.double() * G_UNIT).float(),
                           w=(sign.double() * 2.0 ** j.double()).float(), mean=mean_i.float().reshape(M), rstd=(2.0 ** -k.double()).float().reshape(M),
                           db=exact_f32(dyi.sum(0), G_UNIT), dw=exact_f32(dw_units.sum(0), 2.0 ** -6))


def ln_dx_rows(case, add=None):
    """The LayerNorm input gradient in fp64: rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * w (+ add)."""
    g = case.dy.double() * case.w.double()
    rs = case.rstd.double().unsqueeze(1)
    xh = (case.x.double() - case.mean.double().unsqueeze(1)) * rs
    dx = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx if add is None else dx + add.double()


def case_seed(*v):
    return sum((i + 1) * int(x) for i, x in enumerate(v)) % 100003


_REDUCE_BUILDERS = {"fwd_partials": fwd_partials, "bwd_partials": bwd_partials, "cancelling": cancelling_partials, "bn_rows": bn_rows_case, "dgrad_bn": dgrad_bn_case,
                    "pooled": pooled_case, "colsum": colsum_case, "ln": ln_case}


@functools.lru_cache(maxsize=1)
def reduce_case(kind, *args):
    """The one instance of a reduction case that the CPU proofs and the GPU tests share: its seed is a function of the arguments.
    Only the most recent case is kept (the largest hold hundreds of MB)."""
    flat = [v for a in args for v in (a if isinstance(a, tuple) else (a,))]
    return _REDUCE_BUILDERS[kind](*args, case_seed(len(kind), *flat))
