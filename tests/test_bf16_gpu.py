"""conv_math="bf16" on the GPU, bit for bit: every one-plane kernel against exact.six_term(A, B, terms=((0, 0),)) -- the hi * hi
product alone -- on the exactly-summable classes of tests/exact.py.  No tolerance.  On SA, SB and SMM that model differs from the
six-product one in more than half of the outputs (test_bf16_cpu.py), so a launch that ran the split kernels fails here, and a
one-plane kernel that reads a wrong plane, row or K stage moves integers on every class."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as X  # noqa: E402
import bf16_model as M  # noqa: E402
from exact import assert_bitwise  # noqa: E402
from test_exact_gpu import _grid_noise, _ids, _mask_src, check_stats, dgrad_case, fwd_case, wgrad_case  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _model(contract, A, B, small):
    """fp32 contraction of the hi planes; on small cases required to equal the fp64 definition."""
    r = contract(M.hi(A), M.hi(B))
    if small:
        assert torch.equal(r.double(), M.one_term(A, B, contract)), "the CPU model is not exact here"
    return r


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", M.GG_BF16, ids=_ids)
def test_gather_gemm_fwd_dgrad_bf16(ops, geom, cls):
    """Forward (+ fused fp64 statistics) and input gradient (plain; + residual + ReLU mask; accumulated in place; a parity-class subset)."""
    N, H, W, Cin, Cout, k, s, p = geom
    x, w, u, _y, _sq = fwd_case(cls, geom)
    con = lambda a, b: X.conv_fwd(a, b, s, p)
    M.assert_hi_budget(x, w, u, contract=con, name=f"fwd {cls} {geom}")
    y_ref = _model(con, x, w, True)
    xd, wd = x.cuda(), w.cuda()
    part = torch.zeros(ops.conv2d_fwd_partial_elems(N, H, W, Cin, Cout, k, k, s, p), device="cuda")
    y, tiles = ops.conv2d_fwd_bf16(xd, ops.conv2d_wimage_bf16(wd, True), wd.shape, s, p, bn_partial=part)
    assert_bitwise(y, y_ref, f"bf16 forward {cls}", u)
    assert X.sums_are_exact(y_ref, u)
    check_stats(part, tiles, Cout, y, u, f"bf16 forward {cls}")
    dy, w2, u, _dx, res, msk = dgrad_case(cls, geom)
    con = lambda a, b: X.conv_dgrad(a, b, (N, H, W, Cin), s, p)
    M.assert_hi_budget(dy, w2, u, contract=con, extra=res, name=f"dgrad + residual {cls} {geom}")
    M.assert_hi_budget(dy, w2, u, contract=con, scale=2.0, name=f"dgrad accumulate {cls} {geom}")
    dx_ref = _model(con, dy, w2, True)
    dyd, w2d, resd, mskd = dy.cuda(), w2.cuda(), res.cuda(), msk.cuda()
    wS = ops.conv2d_wimage_bf16(w2d, False)
    shp = (N, H, W, Cin)
    dx = ops.conv2d_dgrad_bf16(dyd, wS, w2d.shape, shp, s, p)
    assert_bitwise(dx, dx_ref, f"bf16 input gradient {cls}", u)
    dx2 = torch.full_like(dx, float("nan"))
    ops.conv2d_dgrad_bf16(dyd, wS, w2d.shape, shp, s, p, dx=dx2, residual=resd, relu_src=mskd)
    assert_bitwise(dx2, (dx_ref + res) * (msk > 0), f"bf16 input gradient + residual + mask {cls}", u)
    ops.conv2d_dgrad_bf16(dyd, wS, w2d.shape, shp, s, p, dx=dx, residual=dx)
    assert_bitwise(dx, 2 * dx_ref, f"bf16 input gradient accumulated in place {cls}", u)
    if s == 2:      # classes 1-3 into a prefilled buffer, residual on class 3 only (the downsample fold of the encoder's backward)
        odd = torch.zeros((1, H, W, 1))
        odd[:, 1::2, 1::2] = 1.0
        sub_ref = (dx_ref + res * odd) * (msk > 0)
        sub_ref[:, 0::2, 0::2] = 7.0
        dx3 = torch.full(shp, 7.0, device="cuda")
        ops.conv2d_dgrad_bf16(dyd, wS, w2d.shape, shp, s, p, dx=dx3, residual=resd, relu_src=mskd, class_mask=0xE, residual_mask=0x8)
        assert_bitwise(dx3, sub_ref, f"bf16 stride-2 class subset {cls}", u)


def _gelu_checks(y, yg, name):
    """y_gelu against gelu(y) (erf form) of the stored y.  Bound from the formats: gelu = 0.5 u (1 + erf): erf is accurate to a few ulp
    of values near 1 on either side, so 1 + erf carries <= 4 * 2^-24 absolute, times 0.5 |u| per side and two sides: 2^-22 |u|, plus
    the roundings of the products, 2 * 2^-24 |gelu| <= 2^-23 |u|.  Held to 2^-21 |u| (4 ulp of |u|)."""
    yc, gc = y.double().cpu(), yg.double().cpu()
    ref = 0.5 * yc * (1.0 + torch.erf(yc * 0.5 ** 0.5))
    bad = (gc - ref).abs() > 2.0 ** -21 * yc.abs()
    assert not bad.any(), f"{name}: {int(bad.sum())} gelu outputs off by more than 4 ulp of |u|; worst {((gc - ref).abs() / yc.abs().clamp_min(1e-30)).max().item():.3e}"


def _gelu_grad64(u):
    u = u.double()
    return 0.5 * (1.0 + torch.erf(u * 0.5 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2.0 * torch.pi) ** 0.5


def _gelu_bwd_checks(dx, exact, u_src, name):
    """dx = exact * gelu'(u): gelu' = Phi(u) + u phi(u) lies in [-0.13, 1.13]; erff and expf to a few ulp each and three roundings:
    held to 2^-20 |exact| (8 ulp of a factor of size 1)."""
    ref = exact.double() * _gelu_grad64(u_src)
    bad = (dx.double().cpu() - ref).abs() > 2.0 ** -20 * exact.double().abs()
    assert not bad.any(), f"{name}: {int(bad.sum())} outputs off by more than 2^-20 |dy w^T|"


def test_tile_table_is_covered(ops):
    """On this device the shapes below reach all six tiles of the table."""
    seen = {ops.conv2d_tile_bf16(N * H * W, Cout, 9 * Cin) for N, H, W, Cin, Cout, _t in M.TILE_BF16}
    for N, H, W, Cin, Cout, k, s, p in M.GG_BF16:
        seen.add(ops.conv2d_tile_bf16(N * X.conv_out(H, k, s, p) * X.conv_out(W, k, s, p), Cout, k * k * Cin))
    assert seen == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("case", M.TILE_BF16, ids=_ids)
def test_every_tile_bf16(ops, case):
    """The four large tiles (256x128, 192x128, 256x64, 128x64; the other two run in test_gather_gemm_fwd_dgrad_bf16), each on a shape
    the planner gives it, ragged last tile, with every epilogue input the kernel accepts: the 3x3 forward with statistics; the 3x3
    input gradient with residual and ReLU mask; the Linear forward with bias, residual and the GELU second output; the Linear input
    gradient with residual, and with the GELU mask.  Class R (dense, 10-bit operand: bf16_model.dense_r)."""
    N, H, W, Cin, Cout, tile = case
    rows = N * H * W
    assert ops.conv2d_tile_bf16(rows, Cout, 9 * Cin) == tile and ops.conv2d_tile_bf16(rows, Cout, 1 << 30) == tile
    x, w, u, y_ref, w2, dx_ref = M.tile_case(N, H, W, Cin, Cout)
    part = torch.zeros(ops.conv2d_fwd_partial_elems(N, H, W, Cin, Cout, 3, 3, 1, 1), device="cuda")
    xd, wd = x.cuda(), w.cuda()
    y, tiles = ops.conv2d_fwd_bf16(xd, ops.conv2d_wimage_bf16(wd, True), wd.shape, 1, 1, bn_partial=part)
    bm = (256, 128, 128, 64, 256, 192)[tile]
    assert tiles == (rows + bm - 1) // bm and rows % bm != 0
    assert_bitwise(y, y_ref, f"bf16 forward, tile {tile}", u)
    check_stats(part, tiles, Cout, y, u, f"bf16 forward, tile {tile}", X.sums_are_exact(y_ref, u))
    # input gradient on the same tile: x as the output gradient (Cin channels), dx with Cout channels; residual + ReLU mask
    res, msk = _grid_noise((N, H, W, Cout), u, tile + 5), _mask_src((N, H, W, Cout), tile + 6)
    w2d = w2.cuda()
    dx = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    ops.conv2d_dgrad_bf16(xd, ops.conv2d_wimage_bf16(w2d, False), w2d.shape, (N, H, W, Cout), 1, 1, dx=dx, residual=res.cuda(),
                          relu_src=msk.cuda())
    assert_bitwise(dx, (dx_ref + res) * (msk > 0), f"bf16 input gradient + residual + mask, tile {tile}", u)
    del dx
    # Linear over the same rows: K = Cin, N = Cout columns -> the same tile
    wl = w[1, 1].contiguous()
    bias, res2 = _grid_noise((Cout,), u, tile + 1), _grid_noise((rows, Cout), u, tile + 2)
    x2 = x.view(rows, Cin)
    M.assert_hi_budget(x2, wl, u, extra=bias.abs() + res2.abs(), name="linear fwd R")
    yl, ygl = torch.full((rows, Cout), float("nan"), device="cuda"), torch.full((rows, Cout), float("nan"), device="cuda")
    ops.linear_fwd(xd.view(rows, Cin), wl.cuda(), bias.cuda(), yl, 1, rows, Cin, Cout, residual=res2.cuda(), y_gelu=ygl,
                   wsplit=ops.conv2d_wimage_bf16(wl.cuda().view(1, 1, Cin, Cout), True), bf16=True)
    assert_bitwise(yl, M.hi(x2) @ M.hi(wl) + bias + res2, f"bf16 linear fwd + bias + residual, tile {tile}", u)
    _gelu_checks(yl, ygl, f"bf16 linear fwd gelu output, tile {tile}")
    # Linear input gradient [rows][N'] x [N'][K'] -> K' = Cout columns: the same tile; N' = Cin
    wl2 = w2[1, 1].contiguous()                                   # [K' = Cout][N' = Cin]
    add = _grid_noise((rows, Cout), u, tile + 3)
    prod = M.hi(x2) @ M.hi(wl2).t()
    M.assert_hi_budget(x2, wl2.t(), u, extra=add, name="linear dgrad R")
    wS = ops.conv2d_wimage_bf16(wl2.cuda().view(1, 1, Cout, Cin), False)
    dxl = torch.full((rows, Cout), float("nan"), device="cuda")
    ops.linear_dgrad(xd.view(rows, Cin), wl2.cuda(), dxl, None, 1, rows, Cout, Cin, residual=add.cuda(), wsplit=wS, bf16=True)
    assert_bitwise(dxl, prod + add, f"bf16 linear dgrad + residual, tile {tile}", u)
    usrc = _mask_src((rows, Cout), tile + 4)
    ops.linear_dgrad(xd.view(rows, Cin), wl2.cuda(), dxl, None, 1, rows, Cout, Cin, gelu_src=usrc.cuda(), wsplit=wS, bf16=True)
    _gelu_bwd_checks(dxl, prod, usrc, f"bf16 linear dgrad * gelu', tile {tile}")
    if tile == M.TILE_BF16[-1][-1]:
        M.tile_case.cache_clear()


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("geom", M.WGRAD_BF16, ids=_ids)
def test_wgrad_per_tap_bf16(ops, geom, cls):
    """Per-tap weight gradient, 64x64 and 128x128 tiles, stride 1 and 2: several split-K ranges and a last K stage that is not full."""
    N, H, W, Cin, Cout, k, s, p = geom
    x, dy, u, _dw = wgrad_case(cls, geom)
    con = lambda a, b: X.conv_wgrad(a, b, k, s, p)
    M.assert_hi_budget(x, dy, u, contract=con, name=f"wgrad {cls} {geom}")
    dw_ref = _model(con, x, dy, True)
    nbytes = ops.conv2d_wgrad_ws_bytes_bf16(N, H, W, Cin, Cout, k, k, s, p)
    pixels = dy.numel() // Cout
    assert nbytes // (k * k * Cin * Cout * 4) >= 2 and pixels % 32 != 0, "the case must force split-K ranges and a remainder"
    ws = torch.empty(nbytes // 4, device="cuda")
    dw = torch.full((k, k, Cin, Cout), float("nan"), device="cuda")
    ops.conv2d_wgrad_bf16(x.cuda(), dy.cuda(), dw, s, p, ws)
    assert_bitwise(dw, dw_ref, f"bf16 per-tap weight gradient {cls}", u)


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", M.LINEAR_BF16, ids=_ids)
def test_linear_bf16(ops, case, cls):
    """Linear forward (+ bias + residual; rows outside the window untouched), input gradient (+ residual), weight gradient and the
    bias gradient out of the same pass (fp32 column sums of dy: exact wherever dy's own sums are)."""
    groups, rows, xg, xo, yg, yo, K, N = case
    sd = M.seed_of(*case) + 11
    (x, w, u), (dy, w2, u2), (x3, dy3, u3) = M.linear_case(cls, case)
    bias, res = _grid_noise((N,), u, sd + 1), _grid_noise((groups, yg, N), u, sd + 2)
    xs = x[:, xo:xo + rows]
    win = slice(yo, yo + rows)
    M.assert_hi_budget(xs, w, u, extra=bias.abs() + res[:, win].abs(), name=f"linear fwd {cls}")
    y_ref = _model(lambda a, b: a @ b, xs, w, True)
    wd = w.cuda()
    wT = ops.conv2d_wimage_bf16(wd.view(1, 1, K, N), True)
    kw = dict(x_group_rows=xg, x_off=xo, y_group_rows=yg, y_off=yo, wsplit=wT, bf16=True)
    y = torch.full((groups, yg, N), 7.0, device="cuda")
    ops.linear_fwd(x.cuda(), wd, None, y, groups, rows, K, N, **kw)
    assert_bitwise(y[:, win], y_ref, f"bf16 linear fwd {cls}", u)
    y2 = torch.full((groups, yg, N), 7.0, device="cuda")
    ops.linear_fwd(x.cuda(), wd, bias.cuda(), y2, groups, rows, K, N, residual=res.cuda(), **kw)
    assert_bitwise(y2[:, win], y_ref + bias + res[:, win], f"bf16 linear fwd + bias + residual {cls}", u)
    for t in (y, y2):
        assert torch.all(t[:, :yo] == 7.0) and torch.all(t[:, yo + rows:] == 7.0), "rows outside the window must stay untouched"
    y3, yg3 = torch.full((groups, yg, N), 7.0, device="cuda"), torch.full((groups, yg, N), 7.0, device="cuda")
    ops.linear_fwd(x.cuda(), wd, bias.cuda(), y3, groups, rows, K, N, y_gelu=yg3, **kw)
    assert_bitwise(y3[:, win], y_ref + bias, f"bf16 linear fwd + bias with the gelu output {cls}", u)
    _gelu_checks(y3[:, win], yg3[:, win], f"bf16 linear fwd gelu output {cls}")
    assert torch.all(yg3[:, :yo] == 7.0) and torch.all(yg3[:, yo + rows:] == 7.0), "gelu rows outside the window must stay untouched"
    # input gradient (dense rows): reduction over N
    Mr = groups * rows
    u = u2
    add = _grid_noise((Mr, K), u, sd + 4)
    M.assert_hi_budget(dy, w2.t(), u, extra=add, name=f"linear dgrad {cls}")
    dx_ref = _model(lambda a, b: a @ b, dy, w2.t(), True)
    w2d = w2.cuda()
    wS = ops.conv2d_wimage_bf16(w2d.view(1, 1, K, N), False)
    dx = torch.full((Mr, K), float("nan"), device="cuda")
    ops.linear_dgrad(dy.cuda(), w2d, dx, None, 1, Mr, K, N, wsplit=wS, bf16=True)
    assert_bitwise(dx, dx_ref, f"bf16 linear dgrad {cls}", u)
    ops.linear_dgrad(dy.cuda(), w2d, dx, None, 1, Mr, K, N, residual=add.cuda(), wsplit=wS, bf16=True)
    assert_bitwise(dx, dx_ref + add, f"bf16 linear dgrad + residual {cls}", u)
    usrc = _mask_src((Mr, K), sd + 6)
    ops.linear_dgrad(dy.cuda(), w2d, dx, None, 1, Mr, K, N, gelu_src=usrc.cuda(), wsplit=wS, bf16=True)
    _gelu_bwd_checks(dx, dx_ref, usrc, f"bf16 linear dgrad * gelu' {cls}")
    # weight gradient + bias gradient: reduction over the rows
    u = u3
    xs3 = x3[:, xo:xo + rows].reshape(Mr, K)
    M.assert_hi_budget(xs3.t(), dy3, u, name=f"linear wgrad {cls}")
    dw_ref = _model(lambda a, b: a @ b, xs3.t(), dy3, True)
    ws = torch.empty(ops.linear_wgrad_ws_bytes(Mr, K, N, bf16=True) // 4 + 4, device="cuda")
    dw, db = torch.full((K, N), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda")
    ops.linear_wgrad(x3.cuda(), dy3.cuda(), dw, ws, groups, rows, K, N, x_group_rows=xg, x_off=xo, dbias=db, bf16=True)
    assert_bitwise(dw, dw_ref, f"bf16 linear wgrad {cls}", u)
    if cls != "SB":                                          # (SB: dy is the dense 18-bit operand, its column sums are not exactly summable)
        ub = X.GRID[X.SPEC[cls][1]]
        X.assert_exact_budget(torch.ones((1, Mr)), dy3, ub, name=f"linear dbias {cls}")
        assert_bitwise(db, dy3.double().sum(0).float(), f"bf16 fused bias gradient {cls}", ub)
    dw2 = torch.full((K, N), float("nan"), device="cuda")
    ops.linear_wgrad(x3.cuda(), dy3.cuda(), dw2, ws, groups, rows, K, N, x_group_rows=xg, x_off=xo, bf16=True)
    assert_bitwise(dw2, dw_ref, f"bf16 linear wgrad without bias {cls}", u)


# ---- one ResNet block, three arithmetics --------------------------------------------------------------------------------------
def _block_ops(ops, math):
    """(weight image or weight, forward, input gradient, weight gradient) of one arithmetic behind one call shape."""
    if math == "f32":
        def dgrad(dy, w, shp, dx, **kw):
            return ops.conv2d_dgrad(dy, w, shp, 1, 1, torch.empty(w.numel(), device="cuda"), dx=dx, **kw)
        return (lambda w, t: w, lambda x, wi, w: ops.conv2d_fwd(x, w, 1, 1)[0], lambda dy, wi, w, shp, dx, **kw: dgrad(dy, w, shp, dx, **kw),
                ops.conv2d_wgrad, ops.conv2d_wgrad_ws_bytes)
    if math == "split":
        return (ops.conv2d_wsplit, lambda x, wi, w: ops.conv2d_fwd_split(x, wi, w.shape, 1, 1)[0],
                lambda dy, wi, w, shp, dx, **kw: ops.conv2d_dgrad_split(dy, wi, w.shape, shp, 1, 1, dx=dx, **kw),
                ops.conv2d_wgrad_split, ops.conv2d_wgrad_split_ws_bytes)
    return (ops.conv2d_wimage_bf16, lambda x, wi, w: ops.conv2d_fwd_bf16(x, wi, w.shape, 1, 1)[0],
            lambda dy, wi, w, shp, dx, **kw: ops.conv2d_dgrad_bf16(dy, wi, w.shape, shp, 1, 1, dx=dx, **kw),
            ops.conv2d_wgrad_bf16, ops.conv2d_wgrad_ws_bytes_bf16)


def test_resnet_block_three_arithmetics_agree(ops):
    """conv - bn - relu - conv (+ identity) - relu, forward and backward, on class-D data kept below 2^8: every operand of every
    contraction is an integer of at most 8 significant bits, which bf16 holds exactly, so f32, split and bf16 must all return the CPU
    fp32 result bit for bit.  The BatchNorms are affine maps with integer parameters (mean 0, invstd 1, gamma 1, integer beta), the
    only BatchNorm that is exact; its backward is then the identity."""
    N, H, W, C = 2, 12, 10, 64
    g = torch.Generator().manual_seed(7)
    tri = lambda *s: torch.randint(-1, 2, s, generator=g).float()
    x, w1, w2, dout = tri(N, H, W, C), tri(3, 3, C, C), tri(3, 3, C, C), tri(N, H, W, C)
    b1, b2 = torch.randint(-3, 4, (C,), generator=g).float(), torch.randint(-3, 4, (C,), generator=g).float()
    # CPU fp32 reference
    y1 = X.conv_fwd(x, w1, 1, 1)
    a1 = torch.relu(y1 + b1)
    y2 = X.conv_fwd(a1, w2, 1, 1)
    out = torch.relu(y2 + b2 + x)
    gout = dout * (out > 0)
    da1 = X.conv_dgrad(gout, w2, (N, H, W, C), 1, 1) * (a1 > 0)
    dw2 = X.conv_wgrad(a1, gout, 3, 1, 1)
    dx = X.conv_dgrad(da1, w1, (N, H, W, C), 1, 1) + gout
    dw1 = X.conv_wgrad(x, da1, 3, 1, 1)
    for nm, t in (("x", x), ("a1", a1), ("gout", gout), ("da1", da1)):
        assert t.abs().max() < 256 and torch.equal(t, M.hi(t)), f"{nm} must be exact in bf16"
    for nm, (a, b, con) in {"y1": (x, w1, lambda a, b: X.conv_fwd(a, b, 1, 1)), "y2": (a1, w2, lambda a, b: X.conv_fwd(a, b, 1, 1)),
                            "dw2": (a1, gout, lambda a, b: X.conv_wgrad(a, b, 3, 1, 1)), "dw1": (x, da1, lambda a, b: X.conv_wgrad(a, b, 3, 1, 1))}.items():
        X.assert_exact_budget(a, b, 1.0, contract=con, name=nm)
    ref = {"out": out, "da1": da1, "dw2": dw2, "dx": dx, "dw1": dw1}
    zero, one = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    xd, w1d, w2d, doutd, b1d, b2d = (t.cuda() for t in (x, w1, w2, dout, b1, b2))
    Mr = N * H * W
    for math in ("f32", "split", "bf16"):
        image, fwd, dgrad, wgrad, ws_bytes = _block_ops(ops, math)
        ws = torch.empty(ws_bytes(N, H, W, C, C, 3, 3, 1, 1) // 4 + 4, device="cuda")
        y1d = fwd(xd, image(w1d, True), w1d)
        a1d = ops.bn_apply(y1d, zero, one, one, b1d, torch.empty_like(y1d), Mr, C, True)
        y2d = fwd(a1d, image(w2d, True), w2d)
        outd = ops.bn_apply(y2d, zero, one, one, b2d, torch.empty_like(y2d), Mr, C, True, residual=xd)
        goutd = doutd * (outd > 0)
        got = {"out": outd}
        got["da1"] = dgrad(goutd, image(w2d, False), w2d, (N, H, W, C), torch.full_like(xd, float("nan")), relu_src=a1d)
        got["dw2"] = wgrad(a1d, goutd, torch.full_like(w2d, float("nan")), 1, 1, ws).clone()
        got["dx"] = dgrad(got["da1"], image(w1d, False), w1d, (N, H, W, C), torch.full_like(xd, float("nan")), residual=goutd)
        got["dw1"] = wgrad(xd, got["da1"], torch.full_like(w1d, float("nan")), 1, 1, ws).clone()
        for k_, v in ref.items():
            assert_bitwise(got[k_], v, f"ResNet block, {math}: {k_}", 1.0)


def test_two_arithmetics_on_two_streams():
    """A split encoder and a bf16 encoder in one process, forward and backward interleaved on two streams: each equals its own
    single-model result bit for bit (the arithmetic is chosen per call; a process-wide switch would cross them over)."""
    from mla_hip.encoder import ResNet18Encoder
    from oracle import mla_oracle as O
    params = O.make_resnet18_params("audio", 9)
    x = O.portable_normal(4, (3, 1, 96, 64), stream=1, mean=-5.081, std=4.4849).cuda()
    dfeat = O.portable_normal(5, (3, 512), stream=2).cuda()

    def make(math):
        e = ResNet18Encoder("audio", device="cuda", seed=0, conv_math=math)
        e.load_state_dict(params)
        return e.train()

    def run(e):
        y = e.forward(x)
        e.backward_from_pooled(dfeat, y.shape[1] * y.shape[2])
        return y

    alone = {}
    for math in ("split", "bf16"):
        e = make(math)
        y = run(e)
        torch.cuda.synchronize()
        alone[math] = (y.clone(), e.grad.clone())
    assert not torch.equal(alone["split"][0], alone["bf16"][0]), "the two arithmetics must differ on dense data"
    encs = {m: make(m) for m in ("split", "bf16")}
    streams = {m: torch.cuda.Stream() for m in encs}
    torch.cuda.synchronize()
    ys = {}
    for _rep in range(2):                                    # twice: the second round overlaps with the first's tail
        for m, e in encs.items():
            with torch.cuda.stream(streams[m]):
                ys[m] = e.forward(x)
        for m, e in encs.items():
            with torch.cuda.stream(streams[m]):
                e.backward_from_pooled(dfeat, ys[m].shape[1] * ys[m].shape[2])
    torch.cuda.synchronize()
    for m, e in encs.items():
        assert_bitwise(ys[m], alone[m][0], f"{m} encoder beside the other: features")
        assert_bitwise(e.grad, alone[m][1], f"{m} encoder beside the other: gradients")
