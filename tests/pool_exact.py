"""Exact inputs and references for the pooling and layout kernels (csrc/pool.hip) and the two stem kernels that fuse BatchNorm into
the max-pool (csrc/bn.hip), in the manner of tests/exact.py: small integers held in fp32, every budget asserted before a launch,
references in integer arithmetic or from ATen on the CPU (test_pool_exact_cpu.py proves the tables, test_pool_exact_gpu.py runs them).

  max-pool      The rule both kernels cite is ATen's: the FIRST maximum in row-major window order, `val > max || isnan(val)` -- so a
                NaN wins over everything before it and stays, and a later NaN replaces it.  F.max_pool2d(return_indices=True) on the
                CPU is that rule; its flat indices become the kernels' codes kh * 3 + kw (exact.pooled_idx_cpu).  window_rule() restates
                it tap by tap, so that the reference has a witness of its own.  The backward is a scatter of an integer gradient with
                at most four addends per pixel.
  average pool  x integers: the sum S over P rows is exact in any order (assert_sum_budget), the kernel's own expression is
                fp32(S) * fp32(1 / P) -- one rounding for the reciprocal, one for the product.
  layout        copies: any distinct-looking values (exact_tokens.patch_image's).
  fused stem    exact.pooled_case at any admitted C: bn(y), the ReLU mask and xhat are exact, the sums are bit-equal to int64.

The grid-stride kernels cap their grids (POOL_CAP, BN_EW_CAP workgroups of 256 threads); each has one case whose work is past the
cap by less than one trip, paired with the largest case of the same family below it (trips())."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import exact as X
from exact import assert_sum_budget, rand_ints

POOL_CAP, BN_EW_CAP, TPB = 16384, 8192, 256          # csrc/pool_args.h: POOL_MAX_BLOCKS, BN_EW_MAX_BLOCKS, POOL_THREADS
INF, NAN = float("inf"), float("nan")


def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def trips(units, cap):
    """Trips of the grid-stride loop of a launch over `units` threads' worth of work (pool_args.h: pool_grid_trips)."""
    grid = min(max(-(-units // TPB), 1), cap)
    return -(-units // (grid * TPB))


def lane_image(shape):
    """Distinct-looking values for the copy kernels (exact_tokens.patch_image)."""
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float64) % 8191 - 4095).float().view(shape)


# ---- max-pool: the rule, its codes, its scatter ----------------------------------------------------------------------------------------
def valid_taps(n):
    """The window offsets k in 0..2 for which some output o has 0 <= 2 o - 1 + k < n."""
    return [k for k in range(3) if any(0 <= 2 * o - 1 + k < n for o in range(pool_out(n)))]


def possible_codes(H, W):
    return sorted(kh * 3 + kw for kh in valid_taps(H) for kw in valid_taps(W))


def codes_of(flat, W):
    """Flat input indices iy * W + ix of F.max_pool2d (NHWC-permuted, [N][OH][OW][C]) -> codes kh * 3 + kw."""
    OH, OW = flat.shape[1], flat.shape[2]
    oy, ox = torch.arange(OH).view(1, -1, 1, 1), torch.arange(OW).view(1, 1, -1, 1)
    code = (flat // W - (oy * 2 - 1)) * 3 + (flat % W - (ox * 2 - 1))
    assert int(code.min()) >= 0 and int(code.max()) <= 8
    return code.to(torch.uint8)


def aten_maxpool(x):
    """x fp32 NHWC on the CPU -> (values fp32 NHWC, codes uint8 NHWC) by ATen's max_pool2d 3x3 / 2 / 1."""
    v, flat = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    return v.permute(0, 2, 3, 1).contiguous(), codes_of(flat.permute(0, 2, 3, 1), x.shape[2]).contiguous()


def window_rule(x):
    """The rule restated tap by tap in row-major order: take the tap if it is the first valid one, or `v > best`, or v is NaN."""
    N, H, W, C = x.shape
    OH, OW = pool_out(H), pool_out(W)
    xp = F.pad(x, (0, 0, 1, 1 + (2 * OW - W), 1, 1 + (2 * OH - H)), value=0.0)
    inside = F.pad(torch.ones((1, H, W, 1), dtype=torch.bool), (0, 0, 1, 1 + (2 * OW - W), 1, 1 + (2 * OH - H)), value=False)
    best = torch.full((N, OH, OW, C), -INF)
    code = torch.full((N, OH, OW, C), 255, dtype=torch.uint8)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            ok = inside[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
            take = ok & ((code == 255) | (v > best) | torch.isnan(v))
            best = torch.where(take, v, best)
            code = torch.where(take, torch.tensor(kh * 3 + kw, dtype=torch.uint8), code)
    return best, code


def scatter_ref(dy_i, code, H, W, dtype=torch.int32):
    """The max-pool backward in integer arithmetic: dx[n][sel(o)][c] += dy[n][o][c], [N][H][W][C] (at most four addends)."""
    N, OH, OW, C = dy_i.shape
    c = code.long()
    oy, ox = torch.arange(OH).view(1, -1, 1, 1), torch.arange(OW).view(1, 1, -1, 1)
    flat = ((oy * 2 - 1 + c // 3) * W + (ox * 2 - 1 + c % 3)).reshape(N, -1, C)
    assert int(flat.min()) >= 0 and int(flat.max()) < H * W
    return torch.zeros((N, H * W, C), dtype=dtype).scatter_add_(1, flat, dy_i.reshape(N, -1, C).to(dtype)).view(N, H, W, C)


GEOM_HW = [(H, W) for H in range(1, 10) for W in range(1, 10)]
MAXPOOL_GEOM = [(2, H, W, 8) for H, W in GEOM_HW]
MAXPOOL_CHANNELS = [(3, 9, 7, C) for C in (4, 64, 128, 512)]
MAXPOOL_TRIP, MAXPOOL_BELOW = (1, 1025, 1025, 64), (1, 1023, 1023, 64)     # forward: 513^2 * 16 = 4 210 704 float4 against 4 194 304
DECISION_SHAPE = (2, 9, 7, 8)
NAN_WINDOW = (2, 1)                                    # (oy, ox) of an interior window of DECISION_SHAPE: rows 3..5, columns 1..3
DECISIONS = ["ties", "constant", "increasing", "decreasing", "neg_inf", "pos_inf_ties", "nan_two"] + [f"nan_tap{k}" for k in range(9)]


def maxpool_units(shape):
    """(forward, backward) float4 elements of one max-pool case."""
    N, H, W, C = shape
    return N * pool_out(H) * pool_out(W) * (C // 4), N * H * W * (C // 4)


def _covering_seed(shape, build, codes_fn):
    """The first seed (of 200 from case_seed) for which every code the geometry can have wins somewhere: the data, not luck, covers them."""
    want = set(possible_codes(shape[1], shape[2]))
    base = X.case_seed(*shape)
    for s in range(200):
        c = build(base + 1009 * s)
        if set(codes_fn(c).unique().tolist()) == want:
            return c
    raise AssertionError(f"{shape}: no seed lets every one of the codes {sorted(want)} win")


def _maxpool_finish(x, seed):
    N, H, W, C = x.shape
    y, code = aten_maxpool(x)
    dy_i = rand_ints(y.shape, -7, 7, seed + 1, nonzero=True, dtype=torch.int8)
    assert_sum_budget(torch.tensor(4 * 7), "max-pool backward")          # a pixel lies in at most four windows
    relu_i = rand_ints(x.shape, -2, 2, seed + 2, dtype=torch.int8)
    return SimpleNamespace(shape=(N, H, W, C), x=x, y=y, code=code, dy_i=dy_i, dy=dy_i.float(), relu_src=relu_i.float())


def _maxpool_ties(shape, seed):
    return _maxpool_finish(rand_ints(shape, -8, 8, seed, dtype=torch.int8).float(), seed)


@functools.lru_cache(maxsize=1)
def maxpool_case(shape):
    """Values in [-8, 8] (17 values over up to 9 taps: the maximum is tied, and not zero, in about one window in six), an integer gradient
    (non-zero, |.| <= 7: at most 4 addends, exact) and a ReLU source in [-2, 2].  The small cases are drawn until every possible code wins."""
    if maxpool_units(shape)[1] > 1 << 20:
        return _maxpool_ties(shape, X.case_seed(*shape))
    return _covering_seed(shape, lambda s: _maxpool_ties(shape, s), lambda c: c.code)


def decision_case(kind):
    """One decision case on DECISION_SHAPE; what it must contain is asserted in test_pool_exact_cpu.py."""
    shape = DECISION_SHAPE
    N, H, W, C = shape
    seed = X.case_seed(len(kind), *[ord(ch) for ch in kind])
    raster = torch.arange(H * W, dtype=torch.float32).view(1, H, W, 1).expand(N, H, W, C)
    if kind == "ties":
        x = rand_ints(shape, -8, 8, seed).float()
    elif kind == "constant":
        x = torch.full(shape, 3.0)
    elif kind == "increasing":
        x = (raster - 30).contiguous()
    elif kind == "decreasing":
        x = (30 - raster).contiguous()
    elif kind == "neg_inf":
        x = torch.full(shape, -INF)
    elif kind == "pos_inf_ties":
        x = rand_ints(shape, -8, 8, seed).float()
        x[torch.rand(shape, generator=torch.Generator().manual_seed(seed + 5)) < 0.4] = INF
    else:
        x = rand_ints(shape, -8, 8, seed).float()
        oy, ox = NAN_WINDOW
        pix = lambda k: (oy * 2 - 1 + k // 3, ox * 2 - 1 + k % 3)
        if kind == "nan_two":
            for k in (2, 6):
                x[:, pix(k)[0], pix(k)[1], :] = NAN
            x[:, pix(7)[0], pix(7)[1], :] = 100.0
        else:
            k = int(kind[-1])
            x[:, pix(k)[0], pix(k)[1], :] = NAN
            # the larger finite value after it: the next tap of the window; behind tap 8 the next pixel of the row, which follows
            # the NaN in the windows (oy, ox + 1) and (oy + 1, ox + 1)
            r, c = pix(k + 1) if k < 8 else (pix(8)[0], pix(8)[1] + 1)
            x[:, r, c, :] = 100.0
    return _maxpool_finish(x.contiguous(), seed)


# ---- average pool ----------------------------------------------------------------------------------------------------------------------
AVG_C = (16, 32, 64, 128, 512, 768, 1024, 2048)
AVG_TRIP, AVG_BELOW = (33, 1024, 512), (32, 1024, 512)          # backward: 33 * 1024 * 128 = 4 325 376 float4 against 4 194 304


def avg_layout(C):
    """(cgpb, nrl, grid.y) of avgpool_fwd_kernel: the largest power of two <= 256 that divides C / 4 (pool_args.h)."""
    c4n, cgpb = C // 4, 256
    while cgpb > 1 and c4n % cgpb:
        cgpb >>= 1
    assert cgpb >= 4
    return cgpb, 256 // cgpb, c4n // cgpb


def avg_rows(C):
    nrl = avg_layout(C)[1]
    return sorted({p for p in (1, nrl - 1, nrl, nrl + 1, 128, 147) if p > 0})


AVG_CASES = [(NB, P, C) for C in AVG_C for P in avg_rows(C) for NB in (1, 3)]


@functools.lru_cache(maxsize=1)
def avg_case(NB, P, C):
    """x integers in [-8, 8]: S exact in any order.  fwd = fp32(S) * fp32(1 / P), the kernel's expression, evaluated in fp32 on the CPU;
    bwd = dy * fp32(1 / P) where the ReLU source is positive."""
    seed = X.case_seed(NB, P, C)
    xi = rand_ints((NB, P, C), -8, 8, seed, dtype=torch.int32)
    assert_sum_budget(xi.abs().sum(1, dtype=torch.int64), f"avgpool {NB}x{P}x{C}")
    S = xi.sum(1, dtype=torch.int64)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(P), dtype=torch.float32)
    dy_i = rand_ints((NB, C), -7, 7, seed + 1, nonzero=True, dtype=torch.int32)
    relu_i = rand_ints((NB, P, C), -2, 2, seed + 2, dtype=torch.int8)
    dy = dy_i.float()
    g = (dy * inv).view(NB, 1, C).expand(NB, P, C)
    return SimpleNamespace(NB=NB, P=P, C=C, x=xi.float(), S=S, inv=inv, fwd=X.exact_f32(S, 1.0) * inv, quot=S.double() / P, dy=dy,
                           relu_src=relu_i.float(), bwd=g.contiguous(), bwd_relu=torch.where(relu_i > 0, g, torch.zeros(())).contiguous())


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
# (B, C, T, H, W); the last one: 28 * 3 * 224 * 224 = 4 214 784 pixels against 16384 * 256 = 4 194 304
VIDEO_CASES = [(2, C, 3, 5, 7) for C in (1, 3, 8)] + [(1, C, 1, 1, 1) for C in (1, 3, 8)]
VIDEO_TRIP, VIDEO_BELOW = (28, 3, 3, 224, 224), (27, 3, 3, 224, 224)
TRANSPOSE_SIZES = (1, 31, 32, 33, 70)
TRANSPOSE_CASES = [(3, R, S) for R in TRANSPOSE_SIZES for S in TRANSPOSE_SIZES]          # (images, R, S): [R][S] -> [S][R]


def video_ref(src):
    B, C, T, H, W = src.shape
    return src.permute(0, 2, 3, 4, 1).reshape(B * T, H, W, C).contiguous()


def split_hw(n):
    """n = H * W with H the largest divisor <= sqrt(n): the transposes only see the product."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


# ---- fused stem ------------------------------------------------------------------------------------------------------------------------
STEM_C = tuple(4 << k for k in range(9))                                    # every C = 4 * 2^k <= 1024 that bn_check admits
STEM_GEOM = [(2, H, W, 8) for H, W in GEOM_HW]
STEM_CHANNELS = [(3, 9, 7, C) for C in STEM_C]
STEM_ROWS = {31: (31, 1, 1, 64), 32: (2, 8, 7, 64), 33: (11, 5, 2, 64), 65: (13, 9, 2, 64)}     # pooled rows: either side of the 32-row tile; tiles that span images
STEM_WS = [(2341, 5, 7, 64), (10891, 1, 5, 64)]        # the tile rule of the pooled rows alone gives more partial rows than ws holds
STEM_FWD_TRIP, STEM_FWD_BELOW = (168, 112, 112, 64), (167, 112, 112, 64)    # 168 * 28 * 28 * 16 = 2 107 392 thread quads against 2 097 152
STEM_BWD_TRIP, STEM_BWD_BELOW = (42, 112, 112, 64), (41, 112, 112, 64)      # 42 * 56 * 56 * 16 pixel quads: the same count


def stem_units(shape):
    """(forward, backward apply) threads of one fused-stem case: a 2x2 block of pooled outputs resp. a 2x2 pixel quad, 4 channels each."""
    N, H, W, C = shape
    return N * ((pool_out(H) + 1) // 2) * ((pool_out(W) + 1) // 2) * (C // 4), N * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4)


def bn_tile_rows(M):
    """csrc/pool_args.h, restated."""
    t = -(-M // 2048) if M > (1 << 18) else -(-M // 1024)
    return min(max(-(-t // 16) * 16, 32), 1024)


def ws_rows(M):
    return -(-M // bn_tile_rows(M))


def stem_case(shape):
    """exact.pooled_case (shared with test_reduce_exact through reduce_case), drawn until every possible code wins at the small shapes."""
    if stem_units(shape)[1] > 1 << 16:
        return X.reduce_case("pooled", *shape)
    return _stem_small(shape)


@functools.lru_cache(maxsize=1)
def _stem_small(shape):
    return _covering_seed(shape, lambda s: X.pooled_case(*shape, s), X.pooled_idx_cpu)


def stem_nan_case():
    """Forward only: the case (3, 9, 7, 64) with NaN planted in y -- one pixel of every image in all channels, scattered single elements."""
    c = X.pooled_case(3, 9, 7, 64, X.case_seed(3, 9, 7, 64, 1))
    y = c.y.clone()
    y[:, 4, 3, :] = NAN
    y[torch.rand(y.shape, generator=torch.Generator().manual_seed(7)) < 0.03] = NAN
    act = torch.relu(X.bn_apply_rows(y, c.ch).float())             # NaN stays NaN through the affine map and the ReLU
    assert torch.equal(torch.isnan(act), torch.isnan(y))
    return SimpleNamespace(N=3, H=9, W=7, C=64, OH=c.OH, OW=c.OW, ch=c.ch, y=y, act=act)


def stem_forward_only(shape, seed=None):
    """The first-trip forward case, too large for int64 / fp64 temporaries: y = mean + d drawn as int8, relu(bn(y)) evaluated in fp32,
    where every step is exact (integers times powers of two below 2^24).  NCHW on the CPU (what max_pool2d wants); the test
    permutes on the device.  Returns y, act (fp32 NCHW), the ATen maxima and codes (NCHW)."""
    N, H, W, C = shape
    ch = X.bn_channels(C, X.case_seed(*shape) if seed is None else seed)
    dev = rand_ints((N, C, H, W), -8, 8, X.case_seed(*shape) + 10, dtype=torch.int8)
    v = lambda t: t.view(1, C, 1, 1)
    y = dev.float() + v(ch.mean)
    act = torch.relu(((y - v(ch.mean)) * v(ch.invstd)) * v(ch.gamma) + v(ch.beta))
    pooled, flat = F.max_pool2d(act, 3, 2, 1, return_indices=True)
    oy, ox = torch.arange(pool_out(H)).view(1, 1, -1, 1), torch.arange(pool_out(W)).view(1, 1, 1, -1)
    code = ((flat // W - (oy * 2 - 1)) * 3 + (flat % W - (ox * 2 - 1))).to(torch.uint8)
    return SimpleNamespace(N=N, H=H, W=W, C=C, ch=ch, y=y, act=act, pooled=pooled, code=code)


def stem_dy_bound(g, y, ch, dgamma, dbeta, M):
    """(reference, tolerance) of the apply pass, element by element, as test_pooled_stem_backward derives its bound: with r = g - a - b,
    a = dbeta / M, b = xhat * dgamma / M, every fp32 rounding of the kernel is relative to one term -- 1 / M, the product with it (a: 2,
    b: 3 with xhat * dg, fused or not), the two subtractions (|g| + |a| and |g| + |a| + |b|); g, xhat and gamma * invstd are exact.
    That is at most 2 |g| + 4 |a| + 4 |b| <= 5 (|g| + |a| + |b|) roundings of 2^-24, times |gamma * invstd| <= 1.  At that test's shapes
    (|g| <= 28, |a| <= 2, |b| <= 28) this is its 2e-5; here the terms of each element are used, because at H, W <= 3 there are as many
    pooled outputs as pixels and |a|, |b| reach 7 and 112."""
    xhat = (y.double() - ch.mean.double()) * ch.invstd.double()
    a, b = dbeta.double() / M, xhat * (dgamma.double() / M)
    scale = (ch.gamma.double() * ch.invstd.double())
    ref = scale * (g.double() - a - b)
    tol = scale.abs() * 5 * 2.0 ** -24 * (g.double().abs() + a.abs() + b.abs())
    return ref, tol
