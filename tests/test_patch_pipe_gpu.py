"""The pipelined main loop of patch_split_kernel<128> / <64> (conv_patch_split.hip), bit for bit, on the exact-sum classes of exact.py.

The loop is unrolled per 32-channel chunk (18 half-steps, fragments read one half-step ahead, the stage barrier inside the last
half-step of a stage, weight loads two stages ahead, the next patch loaded a slot or two per stage), so what can go wrong depends on
the number of chunks, on where a tile ends and on which instantiation runs.  The geometries (N, H, W, Cin, Cout):

    (2,10,6,32,128)    one chunk: no patch reload, the loop body runs once     (2,9,56,32,128)   widest patch of the 128-column kernel
    (2,10,6,64,128)    two chunks                                              (2,9,4,64,128)    W = 4: the tallest patch (402 pixels)
    (1,5,3,96,128)     three chunks, less than one tile                        (2,10,6,128,64)   patch_split_kernel<64>: five two-tap
    (2,20,12,128,128)  one full + one ragged tile                              (2,20,12,32,64)     stages, the ninth tap alone
    (3,7,7,256,256)    a tile spans images, eight chunks

The forward runs at every geometry (Cin = 32, 96: the split forward takes an odd number of 32-channel chunks where this kernel serves
the layer).  The input gradient has Cin GEMM columns and Cout / 32 chunks; the library takes it for Cin % 64 == 0 (the patch kernel
needs whole 64-column tiles), so it runs at the five geometries with Cin in (64, 128, 256) -- there (2,10,6,64,128) and (2,9,4,64,128)
are patch_split_kernel<64> with four chunks and (2,10,6,128,64) is the 128-column kernel with two.  No tolerance anywhere: outputs
equal the CPU fp32 conv2d (exact on these inputs), the fused statistics equal the fp64 sums of the stored y, and the fused
BatchNorm-backward reductions, finalized, equal the exact integer sums."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as X  # noqa: E402
from exact import assert_bitwise  # noqa: E402
from test_exact_gpu import check_stats, dgrad_case, fwd_case  # noqa: E402  (the shared, cached case builders)

CASES = [(2, 10, 6, 32, 128), (2, 10, 6, 64, 128), (1, 5, 3, 96, 128), (2, 20, 12, 128, 128), (3, 7, 7, 256, 256), (2, 9, 56, 32, 128),
         (2, 9, 4, 64, 128), (2, 10, 6, 128, 64), (2, 20, 12, 32, 64)]
DGRAD_CASES = [c for c in CASES if c[3] % 64 == 0]
BN_CASES = [(2, 20, 12, 128, 128), (2, 10, 6, 64, 128)]          # 128-column kernel (two tiles, one ragged) and patch_split_kernel<64>
NAN = float("nan")


def _ids(c):
    return "x".join(map(str, c))


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


@pytest.fixture()
def patch_forced(ops):
    default = ops.conv2d_patch()
    ops.conv2d_patch(2)
    try:
        assert ops.conv2d_patch() == 2
        yield ops
    finally:
        ops.conv2d_patch(default)


def _patch_tiles(case):
    N, H, W, Cin, Cout = case
    assert not (Cin == 64 and Cout == 64), "64 -> 64 runs on the persistent kernel, not on patch_split_kernel"
    return (N * H * W + 255) // 256


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_with_statistics(patch_forced, case, cls):
    ops = patch_forced
    N, H, W, Cin, Cout = case
    geom = case + (3, 1, 1)
    x, w, u, y_ref, sq_exact = fwd_case(cls, geom)
    assert sq_exact, f"{geom} {cls}: sum y^2 is not exact in fp64"
    xd, wd = x.cuda(), w.cuda()
    wT = ops.conv2d_wsplit(wd, True)
    y, _ = ops.conv2d_fwd_split(xd, wT, wd.shape, 1, 1)
    assert_bitwise(y, y_ref, f"patch forward {cls} {geom}", u)
    part = torch.zeros(ops.conv2d_fwd_partial_elems(N, H, W, Cin, Cout, 3, 3, 1, 1), device="cuda")
    y2, tiles = ops.conv2d_fwd_split(xd, wT, wd.shape, 1, 1, y=torch.full_like(y, NAN), bn_partial=part)
    assert tiles == _patch_tiles(case), "the patch kernel did not run"
    assert_bitwise(y2, y_ref, f"patch forward + statistics {cls} {geom}", u)
    check_stats(part, tiles, Cout, y2, u, f"patch forward {cls} {geom}")


@pytest.mark.parametrize("cls", X.CLASSES)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_ids)
def test_input_gradient(patch_forced, case, cls):
    """Plain, with residual + ReLU mask, and accumulated in place (the residual aliases the output)."""
    ops = patch_forced
    N, H, W, Cin, Cout = case
    geom = case + (3, 1, 1)
    dy, w, u, dx_ref, res, msk = dgrad_case(cls, geom)
    dyd, wd, resd, mskd = dy.cuda(), w.cuda(), res.cuda(), msk.cuda()
    wS = ops.conv2d_wsplit(wd, False)
    shape = (N, H, W, Cin)
    dx = ops.conv2d_dgrad_split(dyd, wS, wd.shape, shape, 1, 1)
    assert_bitwise(dx, dx_ref, f"patch input gradient {cls} {geom}", u)
    dx2 = torch.full_like(dx, NAN)
    ops.conv2d_dgrad_split(dyd, wS, wd.shape, shape, 1, 1, dx=dx2, residual=resd, relu_src=mskd)
    assert_bitwise(dx2, (dx_ref + res) * (msk > 0), f"patch input gradient + residual + mask {cls} {geom}", u)
    ops.conv2d_dgrad_split(dyd, wS, wd.shape, shape, 1, 1, dx=dx, residual=dx)
    assert_bitwise(dx, 2 * dx_ref, f"patch input gradient accumulated in place {cls} {geom}", u)


@pytest.mark.parametrize("case", BN_CASES, ids=_ids)
def test_input_gradient_with_bn_requests(patch_forced, case):
    """One and two fused BatchNorm-backward reduction requests (class D operands: the sums are exact integers), with and without
    residual / ReLU mask; the tile count of the partial rows is the patch kernel's."""
    ops = patch_forced
    N, H, W, Cin, Cout = case
    geom = case + (3, 1, 1)
    M = N * H * W
    c = X.reduce_case("dgrad_bn", geom)
    dyd, wd, resd, mskd = c.dy.cuda(), c.w.cuda(), c.res.cuda(), c.msk.cuda()
    zs = [z.cuda() for z in c.zs]
    chs = [(ch.mean.cuda(), ch.invstd.cuda(), ch.gamma.cuda(), ch.beta.cuda()) for ch in c.chs]
    need = ops.conv2d_dgrad_bn_partial_elems(N, H, W, Cin)
    wS = ops.conv2d_wsplit(wd, False)
    for with_res, with_mask, nreq in ((True, True, 1), (True, True, 2), (False, True, 1), (False, False, 2)):
        v_ref = c.dx + c.res if with_res else c.dx.clone()
        if with_mask:
            v_ref = v_ref * (c.msk > 0)
        parts = [torch.full((need,), NAN, device="cuda") for _ in range(nreq)]
        dx, tiles = ops.conv2d_dgrad_split(dyd, wS, wd.shape, (N, H, W, Cin), 1, 1, dx=torch.full((N, H, W, Cin), NAN, device="cuda"),
                                           residual=resd if with_res else None, relu_src=mskd if with_mask else None,
                                           bn_reqs=[(zs[q], chs[q][0], chs[q][1], parts[q]) for q in range(nreq)])
        name = f"patch input gradient {_ids(geom)} residual={with_res} mask={with_mask} requests={nreq}"
        assert tiles == _patch_tiles(case), "the patch kernel did not run"
        assert_bitwise(dx, v_ref, name + ": dx", 1.0)
        for q in range(nreq):
            dg_ref, db_ref = X.dgrad_bn_sums(c, v_ref, q)
            o, dg, db = (torch.full(s, NAN, device="cuda") for s in ((M, Cin), (Cin,), (Cin,)))
            ops.bn_bwd_from_partial(dx.view(M, Cin), zs[q].view(M, Cin), chs[q][0], chs[q][1], chs[q][2], o, dg, db, parts[q], tiles, M, Cin)
            assert_bitwise(db, db_ref, f"{name}: dbeta (request {q})", 1.0)
            assert_bitwise(dg, dg_ref, f"{name}: dgamma (request {q})", 0.125)
            assert not torch.isnan(o).any()
