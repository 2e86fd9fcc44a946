"""CPU model of conv_math="bf16" for the bit-exact tests: y = sum bf16_rne(a) * bf16_rne(b), i.e. the hi * hi product of the split
set alone, exact.six_term(A, B, terms=((0, 0),)).  On the exactly-summable classes of tests/exact.py the sum of |hi(a) * hi(b)|
stays below 2^24 units (test_bf16_cpu.py checks it at every geometry used on the GPU), so a plain CPU fp32 contraction of the two
hi planes IS that model, bit for bit, in any summation order."""
import functools

import torch

import exact as X

ONE = ((0, 0),)

# geometries (N, H, W, Cin, Cout, k, stride, pad) of the gather-GEMM forward / input-gradient cases: 3x3 / 1 / 1, 3x3 / 2, the 1x1 / 2
# downsample, Cin and Cout at 64 and 128, N*H*W = 126 and 1122 (no multiple of any tile; 1122 rows: several tiles), and a 256-channel K loop
GG_BF16 = [(2, 9, 7, 64, 64, 3, 1, 1), (2, 9, 7, 64, 128, 3, 2, 1), (2, 9, 7, 64, 128, 1, 2, 0), (2, 9, 7, 128, 128, 3, 1, 1),
           (2, 33, 17, 128, 128, 3, 1, 1), (2, 10, 8, 128, 256, 3, 2, 1)]
# per-tap weight gradient: 1040 / 1122 / 1300 pixels = several split-K ranges and a last K stage that is not full
WGRAD_BF16 = [(4, 20, 13, 64, 64, 3, 1, 1), (2, 33, 17, 128, 128, 3, 1, 1), (5, 40, 26, 64, 128, 3, 2, 1)]
# Linear: groups, rows, x_group_rows, x_off, y_group_rows, y_off, K, N -- K = N = 64; K = 128 with N = 192; 33 and 257 rows (the
# remainder token); the grouped row offsets of the M3AE image path (y_off = 1 behind the cls token) and a windowed input
LINEAR_BF16 = [(1, 33, 33, 0, 33, 0, 64, 64), (1, 257, 257, 0, 257, 0, 128, 192), (2, 32, 32, 0, 33, 1, 128, 192),
               (2, 33, 35, 1, 36, 2, 64, 128)]
# one shape per tile the planner can pick (index: 256x128, 128x128, 128x64, 64x64, 256x64, 192x128); the 64x64 and 128x128 tiles are
# what GG_BF16 runs on, the four large ones need tens of thousands of rows: (N, H, W, Cin, Cout, tile), 3x3 / 1 / 1
TILE_BF16 = [(4, 127, 127, 64, 128, 0), (3, 127, 127, 64, 128, 5), (8, 125, 131, 64, 64, 4), (4, 125, 131, 64, 64, 2)]


def hi(x):
    return x.float().bfloat16().float()


def one_term(A, B, contract=X.matmul64):
    """The arithmetic's definition: exact.six_term with the hi * hi product alone (fp64)."""
    return X.six_term(A, B, contract=contract, terms=ONE)


def assert_hi_budget(A, B, unit, contract=X.matmul64, extra=None, scale=1.0, name="", fp32_bound=False):
    """sum |hi(a) * hi(b)| (+ |extra|) < 2^24 units: hi rounds upward by up to 2^-8, so the classes' own budget does not carry over."""
    return X.assert_exact_budget(hi(A), hi(B), unit, contract=contract, extra=extra, scale=scale, name=name, fp32_bound=fp32_bound)


def dense_r(shape_a, shape_b, seed):
    """Class R for the tens-of-thousands-of-rows shapes, where the sparse classes' generators cost minutes: A dense multiples of 2^-9
    with |a| < 2 (10 significant bits: hi(a) != a for most), B dense integers |b| <= 3.  Unit 2^-9; K = 576: 576 * 2 * 3 * 2^9 < 2^21."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randint(-(2 ** 10 - 1), 2 ** 10, tuple(shape_a), generator=g).double() * 2.0 ** -9).float()
    B = torch.randint(-3, 4, tuple(shape_b), generator=g).float()
    return A, B, 2.0 ** -9


@functools.lru_cache(maxsize=None)
def tile_case(N, H, W, Cin, Cout):
    """Class-R forward case of one large tile, and the input-gradient case on the same rows AND the same column count (so the same
    tile): x doubles as the output gradient of a 3x3 convolution with Cin output and Cout input channels, dx has Cout channels."""
    x, w, u = dense_r((N, H, W, Cin), (3, 3, Cin, Cout), N * H + W)
    w2 = dense_r((1,), (3, 3, Cout, Cin), N * H + W + 1)[1]
    return x, w, u, X.conv_fwd(hi(x), hi(w), 1, 1), w2, X.conv_dgrad(hi(x), hi(w2), (N, H, W, Cout), 1, 1)


def seed_of(*v):
    return sum((i + 1) * int(x) for i, x in enumerate(v)) % 100003


@functools.lru_cache(maxsize=None)
def linear_case(cls, case):
    """The three contractions of one LINEAR_BF16 case on class cls: forward (x [groups][xg][K], w [K][N]), input gradient
    (dy [M][N], w2 [K][N]) and weight gradient (x3 [groups][xg][K], dy3 [M][N]), each with its unit."""
    groups, rows, xg, xo, yg, yo, K, N = case
    sd = seed_of(*case) + 11
    Mr = groups * rows
    fwd = X.pair(cls, (groups, xg, K), (K, N), sd, axis_a=(2,), axis_b=(0,), forced_a=X.forced_mask((groups, xg, K), (2,), X.k_positions(K), 4),
                 forced_b=X.forced_mask((K, N), (0,), X.k_positions(K), 4))
    dg = X.pair(cls, (Mr, N), (K, N), sd + 3, axis_a=(1,), axis_b=(1,), forced_a=X.forced_mask((Mr, N), (1,), X.k_positions(N), 4),
                forced_b=X.forced_mask((K, N), (1,), X.k_positions(N), 4))
    wg = X.pair(cls, (groups, xg, K), (Mr, N), sd + 5, axis_a=(0, 1), axis_b=(0,),
                forced_a=X.forced_mask((groups, xg, K), (0, 1), X.pixel_positions(groups, xg, 1), 4),
                forced_b=X.forced_mask((Mr, N), (0,), X.pixel_positions(groups, rows, 1), 4))
    return fwd, dg, wg
