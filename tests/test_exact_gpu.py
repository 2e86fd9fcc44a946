"""Every contraction kernel against the exact result, bit for bit, on the exactly-summable input classes of tests/exact.py.

No tolerance: class D (dense small integers) proves indexing, padding, ragged tiles, accumulation and slab reduction at any K; SA,
SB and SMM make the mid / lo planes of one operand, of the other, and the mid*mid cross term reach the output, so a kernel that
loses, doubles or mis-pairs one of the six bf16 products of the split arithmetic differs by hundreds of units.  The reference is
a plain CPU fp32 conv2d / matmul of the same inputs (exact on these inputs: test_exact_cpu.py), cross-checked against fp64 on the
small cases.  Every case checks its fp32 budget (exact.assert_exact_budget) before it launches anything.

Epilogues that are exact on grid data are part of the cases: bias, residual add, ReLU mask, in-place accumulation, rows outside
a window, and the fused fp64 BatchNorm statistics of the forward kernels (sum y and sum y^2 EQUAL the fp64 sums of the stored y).
Left out because they are not exact by nature: the GELU outputs, the stem's deviation-form statistics.  The fused
BatchNorm-backward reductions and every other reduction between the contractions are exact on integer data with an integer mean and a
power-of-two invstd: test_reduce_exact_gpu.py.  What these tests cannot see is the rounding error of dense fp32 accumulation; that stays with the
2e-5 parity tests (test_ops_gpu.py) and with test_conv_split_is_not_reduced_precision (the statistical claim)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as X  # noqa: E402
from exact import assert_bitwise, assert_exact_budget  # noqa: E402

FP64_CHECK_MACS = 3e8          # the fp32 CPU reference is cross-checked against an fp64 evaluation below this many multiply-adds


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _ref(contract, A, B, macs):
    """CPU fp32 reference; on small cases also required to equal the fp64 evaluation (it must, inside the budget)."""
    r = contract(A, B)
    if macs <= FP64_CHECK_MACS:
        assert torch.equal(r.double(), contract(A.double(), B.double())), "CPU fp32 reference is not exact"
    return r


def _grid_noise(shape, unit, seed):
    """Epilogue addends (bias, residual) on the products' grid: integers of up to 19 bits times the unit."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-(2 ** 19), 2 ** 19, tuple(shape), generator=g).double() * unit).float()


def _mask_src(shape, seed):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))


def _seed(*v):
    return sum((i + 1) * int(x) for i, x in enumerate(v)) % 100003


def _ids(c):
    return "x".join(map(str, c))


# ---- case builders (CPU only, cached: one set of inputs serves every tile configuration) ----------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_case(cls, geom):
    N, H, W, Cin, Cout, k, s, p = geom
    K = k * k * Cin
    x, w, u = X.pair(cls, (N, H, W, Cin), (k, k, Cin, Cout), _seed(*geom), count_a=X.window_count(k, s, p), axis_b=(0, 1, 2),
                     forced_a=X.window_forced((N, H, W, Cin)), forced_b=X.forced_mask((k, k, Cin, Cout), (0, 1, 2), X.k_positions(K), 4))
    con = lambda a, b: X.conv_fwd(a, b, s, p)
    macs = N * X.conv_out(H, k, s, p) * X.conv_out(W, k, s, p) * Cout * K
    assert_exact_budget(x, w, u, contract=con, name=f"fwd {cls} {geom}", fp32_bound=macs > FP64_CHECK_MACS)
    y = _ref(con, x, w, macs)
    sq_exact = X.sums_are_exact(y, u)         # sum y^2 reaches 2^53 u^2 only on the largest maps (tens of thousands of rows)
    return x, w, u, y, sq_exact


@functools.lru_cache(maxsize=None)
def dgrad_case(cls, geom):
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = X.conv_out(H, k, s, p), X.conv_out(W, k, s, p)
    dy, w, u = X.pair(cls, (N, OH, OW, Cout), (k, k, Cin, Cout), _seed(*geom) + 1, count_a=X.window_count_t(k, s, p, H, W), count_b=X.tap_class_count(s),
                      forced_a=X.window_forced((N, OH, OW, Cout)),
                      forced_b=X.forced_mask((k, k, Cin, Cout), (0, 1, 3), X.k_positions(k * k * Cout), 4))
    con = lambda a, b: X.conv_dgrad(a, b, (N, H, W, Cin), s, p)
    res = _grid_noise((N, H, W, Cin), u, _seed(*geom) + 2)
    msk = _mask_src((N, H, W, Cin), _seed(*geom) + 3)
    macs = N * H * W * Cin * k * k * Cout
    big = macs > FP64_CHECK_MACS
    assert_exact_budget(dy, w, u, contract=con, extra=res, name=f"dgrad+residual {cls} {geom}", fp32_bound=big)
    assert_exact_budget(dy, w, u, contract=con, scale=2.0, name=f"dgrad accumulate {cls} {geom}", fp32_bound=big)
    dx = _ref(con, dy, w, macs)
    return dy, w, u, dx, res, msk


@functools.lru_cache(maxsize=None)
def wgrad_case(cls, geom):
    N, H, W, Cin, Cout, k, s, p = geom
    OH, OW = X.conv_out(H, k, s, p), X.conv_out(W, k, s, p)
    x, dy, u = X.pair(cls, (N, H, W, Cin), (N, OH, OW, Cout), _seed(*geom) + 4, axis_a=(0, 1, 2), axis_b=(0, 1, 2),
                      forced_a=X.forced_mask((N, H, W, Cin), (0, 1, 2), X.pixel_positions(N, H, W), 4),
                      forced_b=X.forced_mask((N, OH, OW, Cout), (0, 1, 2), X.pixel_positions(N, OH, OW), 4))
    con = lambda a, b: X.conv_wgrad(a, b, k, s, p)
    macs = N * OH * OW * Cout * k * k * Cin
    assert_exact_budget(x, dy, u, contract=con, name=f"wgrad {cls} {geom}", fp32_bound=macs > FP64_CHECK_MACS)
    dw = _ref(con, x, dy, macs)
    return x, dy, u, dw


def check_stats(part, tiles, Cout, y, u, name, sq_exact=True):
    """Fused fp64 BatchNorm statistics: the per-tile rows add up to exactly the fp64 sums of the stored y (integers below 2^53).
    sq_exact=False (fwd_case: sum y^2 itself is not representable in fp64): the squares are held to 1e-12, four thousand ulps."""
    pt = part.view(torch.float64)[:tiles * 2 * Cout].view(tiles, 2, Cout).sum(0).cpu()
    yd = y.double().cpu().reshape(-1, Cout)
    assert_bitwise(pt[0], yd.sum(0), name + ": fused sum y", u)
    if sq_exact:
        assert_bitwise(pt[1], (yd * yd).sum(0), name + ": fused sum y^2", u * u)
    else:
        sq = (yd * yd).sum(0)
        assert ((pt[1] - sq).abs() <= 1e-12 * sq).all(), name + ": fused sum y^2"


def run_fwd_dgrad_split(ops, cls, geom, name, stats=True):
    """Forward (+ statistics) and input gradient (plain; + residual + ReLU mask; accumulated in place) of the split kernels that the
    hooks currently select, against the exact results."""
    N, H, W, Cin, Cout, k, s, p = geom
    x, w, u, y_ref, sq_exact = fwd_case(cls, geom)
    xd, wd = x.cuda(), w.cuda()
    part = torch.zeros(ops.conv2d_fwd_partial_elems(N, H, W, Cin, Cout, k, k, s, p), device="cuda")
    y, tiles = ops.conv2d_fwd_split(xd, ops.conv2d_wsplit(wd, True), wd.shape, s, p, bn_partial=part if stats else None)
    assert_bitwise(y, y_ref, f"{name} forward {cls}", u)
    if stats:
        assert sq_exact or N * H * W > 20000, f"{name} {cls} {geom}: sum y^2 is not exact in fp64"
        check_stats(part, tiles, Cout, y, u, f"{name} forward {cls}", sq_exact)
    dy, w2, u, dx_ref, res, msk = dgrad_case(cls, geom)
    dyd, w2d, resd, mskd = dy.cuda(), w2.cuda(), res.cuda(), msk.cuda()
    wS = ops.conv2d_wsplit(w2d, False)
    dx = ops.conv2d_dgrad_split(dyd, wS, w2d.shape, (N, H, W, Cin), s, p)
    assert_bitwise(dx, dx_ref, f"{name} input gradient {cls}", u)
    dx2 = torch.full_like(dx, float("nan"))
    ops.conv2d_dgrad_split(dyd, wS, w2d.shape, (N, H, W, Cin), s, p, dx=dx2, residual=resd, relu_src=mskd)
    assert_bitwise(dx2, (dx_ref + res) * (msk > 0), f"{name} input gradient + residual + mask {cls}", u)
    ops.conv2d_dgrad_split(dyd, wS, w2d.shape, (N, H, W, Cin), s, p, dx=dx, residual=dx)
    assert_bitwise(dx, 2 * dx_ref, f"{name} input gradient accumulated in place {cls}", u)
    return tiles


# every channel pairing of ResNet-18 at reduced spatial size (M = 126: ragged against every tile), plus 1122 rows (several ragged tiles)
GG_CASES = [
    (2, 9, 7, 64, 64, 3, 1, 1), (2, 9, 7, 64, 128, 3, 2, 1), (2, 9, 7, 64, 128, 1, 2, 0), (2, 9, 7, 128, 128, 3, 1, 1),
    (2, 10, 8, 128, 256, 3, 2, 1), (2, 10, 8, 128, 256, 1, 2, 0), (2, 9, 7, 256, 256, 3, 1, 1), (2, 9, 7, 256, 512, 3, 2, 1),
    (2, 9, 7, 256, 512, 1, 2, 0), (2, 9, 7, 512, 512, 3, 1, 1), (2, 33, 17, 128, 128, 3, 1, 1),
]


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5], ids=lambda c: f"tile{c}")
@pytest.mark.parametrize("geom", GG_CASES, ids=_ids)
def test_gather_gemm_fwd_dgrad(ops, geom, cfg, cls):
    """Gather-GEMM forward / input gradient, split arithmetic: the planner's tile (-1; one launch per parity class at stride 2) and every
    forced tile configuration 0..5."""
    default = ops.conv2d_patch()
    ops.conv2d_split_cfg(cfg)
    ops.conv2d_patch(0)
    ops.conv2d_dgrad_merge(0)
    try:
        run_fwd_dgrad_split(ops, cls, geom, f"gather-GEMM tile {cfg}")
    finally:
        ops.conv2d_split_cfg(-1)
        ops.conv2d_patch(default)
        ops.conv2d_dgrad_merge(1)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", [(2, 33, 17, 128, 128, 3, 1, 1), (2, 9, 7, 64, 128, 3, 2, 1)], ids=_ids)
def test_split_terms_controls(ops, geom, cls):
    """The inputs have power ON THE DEVICE: the three-product set (bf16x3) gives a wrong result on SA, SB and SMM and the exact one on
    D (only hi*hi is non-zero there); the eight-product set adds two products that are zero."""
    N, H, W, Cin, Cout, k, s, p = geom
    x, w, u, y_ref, sq_exact = fwd_case(cls, geom)
    dy, w2, u, dx_ref, _, _ = dgrad_case(cls, geom)
    xd, wT, dyd, wS = x.cuda(), ops.conv2d_wsplit(w.cuda(), True), dy.cuda(), ops.conv2d_wsplit(w2.cuda(), False)
    default = ops.conv2d_patch()
    got = {}
    try:
        ops.conv2d_patch(0)
        for terms in (3, 8):
            assert ops.conv2d_split_terms(terms) == terms
            got[terms] = (ops.conv2d_fwd_split(xd, wT, w.shape, s, p)[0].cpu(), ops.conv2d_dgrad_split(dyd, wS, w.shape, (N, H, W, Cin), s, p).cpu())
    finally:
        ops.conv2d_split_terms(6)
        ops.conv2d_patch(default)
    assert_bitwise(got[8][0], y_ref, f"eight products, forward {cls}", u)
    assert_bitwise(got[8][1], dx_ref, f"eight products, input gradient {cls}", u)
    if cls == "D":
        assert_bitwise(got[3][0], y_ref, "three products, forward D", u)
        assert_bitwise(got[3][1], dx_ref, "three products, input gradient D", u)
    else:
        for g, r, nm in ((got[3][0], y_ref, "forward"), (got[3][1], dx_ref, "input gradient")):
            frac = (g != r).double().mean().item()
            assert frac >= 0.25, f"three products, {nm} {cls}: only {frac:.1%} of the outputs differ from the exact result"


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", [(2, 20, 12, 64, 128, 3, 2, 1), (3, 7, 7, 256, 512, 3, 2, 1), (5, 9, 11, 64, 128, 3, 2, 1), (3, 14, 14, 128, 256, 3, 2, 1)],
                         ids=_ids)
def test_merged_stride2_dgrad(ops, geom, cls):
    """Stride-2 input gradient: the four parity classes in one launch and one launch per class, odd and even H / W; and a class subset
    (classes 1-3, residual on class 3 only) into a prefilled buffer."""
    N, H, W, Cin, Cout, k, s, p = geom
    dy, w, u, dx_ref, res, msk = dgrad_case(cls, geom)
    dyd, wd, resd, mskd = dy.cuda(), w.cuda(), res.cuda(), msk.cuda()
    wS = ops.conv2d_wsplit(wd, False)
    odd = torch.zeros((1, H, W, 1))
    odd[:, 1::2, 1::2] = 1.0
    sub_ref = (dx_ref + res * odd) * (msk > 0)
    sub_ref[:, 0::2, 0::2] = 7.0
    assert ops.conv2d_dgrad_merge() == 1
    try:
        for merge in (1, 0):
            ops.conv2d_dgrad_merge(merge)
            dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
            ops.conv2d_dgrad_split(dyd, wS, wd.shape, (N, H, W, Cin), 2, 1, dx=dx, residual=resd, relu_src=mskd)
            assert_bitwise(dx, (dx_ref + res) * (msk > 0), f"stride-2 input gradient, merge={merge} {cls}", u)
            dx2 = torch.full((N, H, W, Cin), 7.0, device="cuda")
            ops.conv2d_dgrad_split(dyd, wS, wd.shape, (N, H, W, Cin), 2, 1, dx=dx2, residual=resd, relu_src=mskd, class_mask=0xE, residual_mask=0x8)
            assert_bitwise(dx2, sub_ref, f"stride-2 class subset, merge={merge} {cls}", u)
    finally:
        ops.conv2d_dgrad_merge(1)


@pytest.mark.parametrize("cls", ["D", "SMM"])
def test_two_phase_launch(ops, cls):
    """A shape the planner splits into whole rounds of a big tile + one launch for the remaining rows (test_conv_two_phase_launch):
    both schedules give the exact result, statistics rows included."""
    geom = (48, 28, 28, 256, 256, 3, 1, 1)
    default = ops.conv2d_patch()
    assert ops.conv2d_two_phase() == 1
    tiles = {}
    try:
        ops.conv2d_patch(0)
        for tp in (1, 0):
            ops.conv2d_two_phase(tp)
            tiles[tp] = run_fwd_dgrad_split(ops, cls, geom, f"two-phase={tp}")
    finally:
        ops.conv2d_two_phase(1)
        ops.conv2d_patch(default)
        fwd_case.cache_clear()
        dgrad_case.cache_clear()
    assert tiles[1] != tiles[0], "the planner was expected to split this shape"


PATCH_EXACT = [
    # (N, H, W, Cin, Cout), classes: the geometry classes of PATCH_CASES (test_ops_gpu.py)
    ((2, 20, 12, 64, 64), X.CLASSES),        # persistent 64 -> 64 kernel, one full + one ragged 256-pixel tile
    ((2, 10, 6, 128, 128), X.CLASSES),       # 128-column kernel
    ((3, 7, 7, 256, 256), X.CLASSES),        # a tile spans several images
    ((2, 4, 4, 512, 512), X.CLASSES),
    ((5, 32, 4, 64, 64), X.CLASSES),         # narrow maps
    ((1, 5, 3, 64, 128), X.CLASSES),         # smaller than one tile
    ((40, 14, 14, 256, 256), ("D", "SMM")),  # many tiles
    ((25, 56, 56, 64, 64), ("D", "SMM")),    # persistent kernel: 307 tiles on 256 workgroups, ragged last tile
]


@pytest.mark.parametrize("case,cls", [(c, k) for c, ks in PATCH_EXACT for k in ks], ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_patch_fwd_dgrad(ops, case, cls):
    """LDS-patch forward / input gradient (128-column and persistent 64 -> 64 kernels), forced wherever the geometry allows."""
    N, H, W, Cin, Cout = case
    geom = case + (3, 1, 1)
    default = ops.conv2d_patch()
    ops.conv2d_patch(2)
    try:
        tiles = run_fwd_dgrad_split(ops, cls, geom, "LDS-patch")
    finally:
        ops.conv2d_patch(default)
        if N * H * W > 5000 and cls == "SMM":
            fwd_case.cache_clear()
            dgrad_case.cache_clear()
    ntiles = (N * H * W + 255) // 256
    assert tiles == (min(ntiles, 256) if (Cin == 64 and Cout == 64 and ntiles >= 2) else ntiles), "the patch kernel did not run"


WGRAD_PT = [(4, 20, 12, 64, 64, 3, 1, 1), (2, 33, 17, 128, 128, 3, 1, 1), (2, 20, 12, 64, 128, 3, 2, 1), (2, 20, 12, 64, 128, 1, 2, 0),
            (3, 14, 14, 128, 256, 3, 2, 1), (3, 14, 14, 128, 256, 1, 2, 0), (3, 7, 7, 256, 512, 3, 2, 1), (2, 9, 7, 512, 512, 3, 1, 1)]
WGRAD_TR = [(2, 20, 12, 64, 64), (5, 9, 11, 64, 64), (1, 8, 8, 64, 64), (2, 28, 28, 128, 128), (3, 14, 14, 256, 256), (2, 16, 8, 128, 256),
            (1, 5, 3, 128, 128), (4, 32, 4, 512, 512), (3, 3, 1, 128, 128)]


def _wgrad_split(ops, cls, geom, name):
    N, H, W, Cin, Cout, k, s, p = geom
    x, dy, u, dw_ref = wgrad_case(cls, geom)
    ws = torch.empty(ops.conv2d_wgrad_split_ws_bytes(N, H, W, Cin, Cout, k, k, s, p) // 4 + 4, device="cuda")
    dw = torch.full((k, k, Cin, Cout), float("nan"), device="cuda")
    ops.conv2d_wgrad_split(x.cuda(), dy.cuda(), dw, s, p, ws)
    assert_bitwise(dw, dw_ref, f"{name} {cls}", u)
    return dw


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", WGRAD_PT, ids=_ids)
def test_wgrad_per_tap(ops, geom, cls):
    """Per-tap weight gradient (128x128 / 64x64 tiles) with its split-K slab reduction, stride 1 and 2, 1x1 downsample."""
    ops.conv2d_wgrad_tr(0)
    try:
        _wgrad_split(ops, cls, geom, "per-tap weight gradient")
    finally:
        ops.conv2d_wgrad_tr(1)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", WGRAD_TR, ids=_ids)
def test_wgrad_all_taps(ops, case, cls):
    """All-taps weight gradient: 8x8-tile kernel (64 -> 64) and flat-tile kernel (128..512 channels); ragged last tile, 4- and 1-pixel-wide
    maps.  The per-tap kernel gives the same (exact) bits here, so that the kernel under test ran is shown by test_wgrad_all_taps_tr_kernel."""
    assert ops.conv2d_wgrad_tr() == 1
    _wgrad_split(ops, cls, case + (3, 1, 1), "all-taps weight gradient")


STEM_EXACT = [(2, 40, 24, 1), (3, 36, 36, 3), (1, 7, 9, 3), (70, 96, 33, 1), (48, 96, 64, 3)]   # the last two: more tiles than workgroups


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("case", STEM_EXACT, ids=_ids)
def test_stem_fwd_wgrad(ops, case, waves, cls):
    """7x7 / 2 / 3 stem, split arithmetic: forward on both workgroup shapes, and the weight gradient."""
    N, H, W, Cin = case
    geom = (N, H, W, Cin, 64, 7, 2, 3)
    x, w, u, y_ref, sq_exact = fwd_case(cls, geom)
    ops.conv2d_stem_waves(waves)
    try:
        y, _ = ops.conv2d_stem_fwd_split(x.cuda(), w.cuda())
    finally:
        ops.conv2d_stem_waves(0)
    assert_bitwise(y, y_ref, f"stem forward, {waves} waves {cls}", u)
    if waves == 4:
        x3, dy, u, dw_ref = wgrad_case(cls, geom)
        dw = torch.full((7, 7, Cin, 64), float("nan"), device="cuda")
        ws = torch.empty(ops.conv2d_stem_wgrad_split_ws_bytes(Cin) // 4, device="cuda")
        ops.conv2d_stem_wgrad_split(x3.cuda(), dy.cuda(), dw, 2, 3, ws)
        assert_bitwise(dw, dw_ref, f"stem weight gradient {cls}", u)
    if waves == 8 and N > 8 and cls == "SMM":
        fwd_case.cache_clear()
        wgrad_case.cache_clear()


@pytest.mark.parametrize("cls", ["D", "SA"])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3], ids=lambda c: f"f32tile{c}")
@pytest.mark.parametrize("geom", [(2, 33, 17, 128, 128, 3, 1, 1), (2, 9, 7, 64, 128, 3, 2, 1), (2, 9, 7, 256, 512, 1, 2, 0), (2, 20, 12, 3, 64, 7, 2, 3)], ids=_ids)
def test_f32_mfma_conv(ops, geom, cfg, cls):
    """The exact-fp32 MFMA kernels -- the comparator of the accuracy claim -- held to the same bar: forward (+ statistics), input and weight
    gradient on every tile."""
    N, H, W, Cin, Cout, k, s, p = geom
    x, w, u, y_ref, sq_exact = fwd_case(cls, geom)
    ops.conv2d_f32_cfg(cfg)
    try:
        part = torch.zeros(ops.conv2d_fwd_partial_elems(N, H, W, Cin, Cout, k, k, s, p), device="cuda")
        y, tiles = ops.conv2d_fwd(x.cuda(), w.cuda(), s, p, bn_partial=part)
        assert_bitwise(y, y_ref, f"fp32 forward {cls}", u)
        check_stats(part, tiles, Cout, y, u, f"fp32 forward {cls}", sq_exact)
        x3, dy3, u, dw_ref = wgrad_case(cls, geom)
        ws = torch.empty(ops.conv2d_wgrad_ws_bytes(N, H, W, Cin, Cout, k, k, s, p) // 4 + 4, device="cuda")
        dw = torch.full((k, k, Cin, Cout), float("nan"), device="cuda")
        ops.conv2d_wgrad(x3.cuda(), dy3.cuda(), dw, s, p, ws)
        assert_bitwise(dw, dw_ref, f"fp32 weight gradient {cls}", u)
        if Cin % 64 == 0:
            dy, w2, u, dx_ref, res, msk = dgrad_case(cls, geom)
            wt_ws = torch.empty(w2.numel(), device="cuda")
            dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
            ops.conv2d_dgrad(dy.cuda(), w2.cuda(), (N, H, W, Cin), s, p, wt_ws, dx=dx, residual=res.cuda(), relu_src=msk.cuda())
            assert_bitwise(dx, (dx_ref + res) * (msk > 0), f"fp32 input gradient + residual + mask {cls}", u)
            ops.conv2d_dgrad(dy.cuda(), w2.cuda(), (N, H, W, Cin), s, p, wt_ws, dx=dx)
            ops.conv2d_dgrad(dy.cuda(), w2.cuda(), (N, H, W, Cin), s, p, wt_ws, dx=dx, residual=dx)
            assert_bitwise(dx, 2 * dx_ref, f"fp32 input gradient accumulated in place {cls}", u)
    finally:
        ops.conv2d_f32_cfg(-1)


# ---- Linear ---------------------------------------------------------------------------------------------------------------------
LINEAR_EXACT = [
    # groups, rows, x_group_rows, x_off, y_group_rows, y_off, K, N
    (2, 130, 131, 1, 132, 2, 768, 384),      # windowed rows: per-tap weight gradient
    (1, 300, 300, 0, 300, 0, 3072, 768),     # dense rows, K = 3072: the 192 x 192 transposing weight-gradient kernel
    (1, 771, 771, 0, 771, 0, 768, 3072),
    (2, 5, 9, 3, 7, 2, 64, 128),
]


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("math_", ["split", "f32"])
@pytest.mark.parametrize("case", LINEAR_EXACT, ids=_ids)
def test_linear_fwd_dgrad(ops, case, math_, cls):
    """Linear forward (+ bias, + residual, windowed rows stay untouched) and input gradient (+ residual), split and fp32 arithmetic."""
    groups, rows, xg, xo, yg, yo, K, N = case
    sd = _seed(*case)
    x, w, u = X.pair(cls, (groups, xg, K), (K, N), sd, axis_a=(2,), axis_b=(0,), forced_a=X.forced_mask((groups, xg, K), (2,), X.k_positions(K), 4),
                     forced_b=X.forced_mask((K, N), (0,), X.k_positions(K), 4))
    bias, res = _grid_noise((N,), u, sd + 1), _grid_noise((groups, yg, N), u, sd + 2)
    xs = x[:, xo:xo + rows]
    win = slice(yo, yo + rows)
    assert_exact_budget(xs, w, u, extra=bias.abs() + res[:, win].abs(), name=f"linear fwd {cls}")
    y_ref = _ref(lambda a, b: a @ b, xs, w, groups * rows * K * N)
    wd = w.cuda()
    wT = ops.conv2d_wsplit(wd.view(1, 1, K, N), True) if math_ == "split" else None
    kw = dict(x_group_rows=xg, x_off=xo, y_group_rows=yg, y_off=yo, wsplit=wT)
    y = torch.full((groups, yg, N), 7.0, device="cuda")
    ops.linear_fwd(x.cuda(), wd, None, y, groups, rows, K, N, **kw)
    assert_bitwise(y[:, win], y_ref, f"linear fwd ({math_}) {cls}", u)
    y2 = torch.full((groups, yg, N), 7.0, device="cuda")
    ops.linear_fwd(x.cuda(), wd, bias.cuda(), y2, groups, rows, K, N, residual=res.cuda(), **kw)
    assert_bitwise(y2[:, win], y_ref + bias + res[:, win], f"linear fwd + bias + residual ({math_}) {cls}", u)
    for t in (y, y2):
        assert torch.all(t[:, :yo] == 7.0) and torch.all(t[:, yo + rows:] == 7.0), "rows outside the window must stay untouched"
    # input gradient (dense rows): reduction over N
    M = groups * rows
    dy, w2, u = X.pair(cls, (M, N), (K, N), sd + 3, axis_a=(1,), axis_b=(1,), forced_a=X.forced_mask((M, N), (1,), X.k_positions(N), 4),
                       forced_b=X.forced_mask((K, N), (1,), X.k_positions(N), 4))
    add = _grid_noise((M, K), u, sd + 4)
    assert_exact_budget(dy, w2.t(), u, extra=add, name=f"linear dgrad {cls}")
    dx_ref = _ref(lambda a, b: a @ b.t(), dy, w2, M * K * N)
    w2d = w2.cuda()
    wS = ops.conv2d_wsplit(w2d.view(1, 1, K, N), False) if math_ == "split" else None
    wt = None if math_ == "split" else torch.empty(K * N, device="cuda")
    dx = torch.full((M, K), float("nan"), device="cuda")
    ops.linear_dgrad(dy.cuda(), w2d, dx, wt, 1, M, K, N, wsplit=wS)
    assert_bitwise(dx, dx_ref, f"linear dgrad ({math_}) {cls}", u)
    ops.linear_dgrad(dy.cuda(), w2d, dx, wt, 1, M, K, N, residual=add.cuda(), wsplit=wS)
    assert_bitwise(dx, dx_ref + add, f"linear dgrad + residual ({math_}) {cls}", u)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("tr", [0, 1], ids=["per-tap", "tr192"])
@pytest.mark.parametrize("case", LINEAR_EXACT, ids=_ids)
def test_linear_wgrad(ops, case, tr, cls):
    """Linear weight gradient on the split arithmetic: the per-tap kernel (forced) and the 192 x 192 transposing kernel (where it applies),
    with the bias gradient out of the same pass: the fused column sums equal the exact ones wherever the budget over the M rows holds
    (SB makes dy the dense 18-bit operand: its column sums are not exactly summable, only dw is checked there); and the fp32 kernel."""
    groups, rows, xg, xo, yg, yo, K, N = case
    sd = _seed(*case) + 5
    M = groups * rows
    x, dy, u = X.pair(cls, (groups, xg, K), (M, N), sd, axis_a=(0, 1), axis_b=(0,),
                      forced_a=X.forced_mask((groups, xg, K), (0, 1), X.pixel_positions(groups, xg, 1), 4),
                      forced_b=X.forced_mask((M, N), (0,), X.pixel_positions(groups, rows, 1), 4))
    xs = x[:, xo:xo + rows].reshape(M, K)
    assert_exact_budget(xs.t(), dy, u, name=f"linear wgrad {cls}")
    dw_ref = _ref(lambda a, b: a.t() @ b, xs, dy, M * K * N)
    ws = torch.empty(ops.linear_wgrad_ws_bytes(M, K, N, True) // 4 + 4, device="cuda")
    dw, db = torch.full((K, N), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda")
    assert ops.conv2d_wgrad_tr() == 1
    ops.conv2d_wgrad_tr(tr)
    try:
        ops.linear_wgrad(x.cuda(), dy.cuda(), dw, ws, groups, rows, K, N, x_group_rows=xg, x_off=xo, split=True, dbias=db)
    finally:
        ops.conv2d_wgrad_tr(1)
    assert_bitwise(dw, dw_ref, f"linear wgrad (split, wgrad_tr={tr}) {cls}", u)
    if cls != "SB":
        ub = X.GRID[X.SPEC[cls][1]]
        assert_exact_budget(torch.ones((1, M)), dy, ub, name=f"linear dbias {cls}")
        assert_bitwise(db, dy.double().sum(0).float(), f"fused bias gradient (wgrad_tr={tr}) {cls}", ub)
    if tr == 0:
        ws32 = torch.empty(ops.linear_wgrad_ws_bytes(M, K, N) // 4 + 4, device="cuda")
        dw32 = torch.full((K, N), float("nan"), device="cuda")
        ops.linear_wgrad(x.cuda(), dy.cuda(), dw32, ws32, groups, rows, K, N, x_group_rows=xg, x_off=xo)
        assert_bitwise(dw32, dw_ref, f"linear wgrad (f32) {cls}", u)


@pytest.mark.parametrize("B,H,n,hd", [(2, 3, 50, 64), (1, 2, 130, 32), (2, 12, 257, 64)])
def test_bgemm_stride_patterns(ops, B, H, n, hd):
    """The six strided batched GEMMs of the attention forward / backward (test_attention_pieces) on class D: any stride mix-up, ragged
    tile or offset error moves integers."""
    D = H * hd
    g = torch.Generator().manual_seed(n)
    ri = lambda *s: torch.randint(-7, 8, s, generator=g).float()
    qkv, P, dO, dP = ri(B, n, 3 * D), ri(B, H, n, n), ri(B, n, D), ri(B, H, n, n)
    q, k_, v = (qkv.view(B, n, 3, H, hd).permute(2, 0, 3, 1, 4)[i] for i in range(3))             # (B, H, n, hd)
    dOh = dO.view(B, n, H, hd).permute(0, 2, 1, 3)
    assert 49 * max(n, hd) < 2 ** 24
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * n, D)
    qd, Pd, dOd, dPd = qkv.cuda().view(B * n, 3 * D), P.cuda(), dO.cuda().view(B * n, D), dP.cuda()
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    qs, ss, os_ = (n * 3 * D, hd, 3 * D, 1), (H * n * n, n * n, n, 1), (n * D, hd, D, 1)
    S = f(B, H, n, n)
    ops.bgemm(qd, qd, S, B, H, n, n, hd, qs, (n * 3 * D, hd, 1, 3 * D), ss, 0.125, b_off=D)
    assert_bitwise(S, 0.125 * (q @ k_.transpose(-2, -1)), "Q K^T", 0.125)
    o = f(B * n, D)
    ops.bgemm(Pd, qd, o, B, H, n, hd, n, ss, (n * 3 * D, hd, 3 * D, 1), os_, 1.0, b_off=2 * D)
    assert_bitwise(o, back(P @ v), "P V", 1.0)
    dPo = f(B, H, n, n)
    ops.bgemm(dOd, qd, dPo, B, H, n, n, hd, os_, (n * 3 * D, hd, 1, 3 * D), ss, 1.0, b_off=2 * D)
    assert_bitwise(dPo, dOh @ v.transpose(-2, -1), "dO V^T", 1.0)
    dqkv = torch.full((B * n, 3 * D), 5.0, device="cuda")
    ops.bgemm(Pd, dOd, dqkv, B, H, n, hd, n, (H * n * n, n * n, 1, n), (n * D, hd, D, 1), qs, 1.0, c_off=2 * D)
    ops.bgemm(dPd, qd, dqkv, B, H, n, hd, n, ss, (n * 3 * D, hd, 3 * D, 1), qs, 0.125, b_off=D)
    ops.bgemm(dPd, qd, dqkv, B, H, n, hd, n, (H * n * n, n * n, 1, n), (n * 3 * D, hd, 3 * D, 1), qs, 0.125, c_off=D)
    want = torch.cat([back(0.125 * (dP @ k_)), back(0.125 * (dP.transpose(-2, -1) @ q)), back(P.transpose(-2, -1) @ dOh)], dim=1)
    assert_bitwise(dqkv, want, "dQ | dK | dV", 0.125)
