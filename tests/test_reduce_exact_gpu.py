"""Every BatchNorm and column-reduction regime against the exact result, on the exactly-summable inputs of tests/exact.py (second half).

The reductions that sit between the contraction kernels -- the BatchNorm statistics and backward sums, their three finalize paths
(one launch up to 1024 tiles, the wide kernel up to 16384, stage 1 + chunk sums beyond), the reductions fused into the input-gradient
epilogue and into the pooled stem backward, the transformer's column sums and LayerNorm affine gradients -- are run at every regime:
each finalize path on both sides of its boundaries and loop tails (on fabricated partial buffers, so 40000 tiles cost a few MB), every
legal channel count, the row edges (M = 1, fewer rows than row lanes, either side of a tile, the tile-rule change above 2^18 rows, the
second trip of the capped elementwise grid).  All sums are required BIT-EQUAL to int64 arithmetic: on integer data a lost, doubled or
mis-paired row, tile or slot is off by whole units.  Every case asserts its 2^24 budget on the CPU before it launches anything
(test_reduce_exact_cpu.py proves the same cases without a GPU); no case is skipped or relaxed.

Integer data cannot see the ORDER of the fp64 additions (every order gives the same bits); test_finalize_order pins it, on the same
finalize cases, with partials whose totals are rounding residue, against the restatement of the kernels' order in tests/exact.py.

What is not exact by nature is held to the formats: invstd and running_var to 2 fp32 ulp of the fp64 evaluation (one correctly rounded
fp64 divide, sqrt and subtract, possibly fused, then one rounding to fp32); the elementwise passes (bn_apply, the BatchNorm and
LayerNorm input gradients) to the fp64 formula at the tolerances of test_bn_fwd_bwd / test_layernorm, element by element, on data
scaled so that a correct kernel cannot miss them (exact.bn_rows_case, exact.ln_case)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as X  # noqa: E402
from exact import assert_bitwise  # noqa: E402

ULP2 = 2.4e-7          # 2 fp32 ulp, relative
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def assert_close_each(got, want, atol, rtol, name):
    """|got - want| <= atol + rtol * |want| for EVERY element (NaN fails); prints the figure before it asserts."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).double()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    ok = err <= tol
    worst = float("inf") if torch.isnan(err).any() else (err / tol.clamp_min(1e-300)).max().item()
    print(f"{name}: worst error / tolerance = {worst:.3g}")
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside atol={atol:g} rtol={rtol:g}; worst error / tolerance = {worst:.3g}"


def _dev_channels(ch):
    return ch.mean.cuda(), ch.invstd.cuda(), ch.gamma.cuda(), ch.beta.cuda()


# ---- 1. finalize regimes on fabricated partials --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,tiles", X.FINALIZE_CASES, ids=_ids)
def test_finalize_forward(ops, C, tiles):
    """mla_bn_finalize on an fp64 [tiles][2][C] buffer of integer sums + its scratch tail, M = 2^k: mean and running_mean bit-equal to
    the fp64 reference rounded to fp32 (s / M and the running-mean update are exact in fp64 on these inputs), invstd and running_var
    within 2 ulp; with and without running statistics."""
    f = X.reduce_case("fwd_partials", tiles, C)
    n = tiles * 2 * C * 2
    buf = _nan(n + ops.bn_partial_scratch_elems(C))            # a scratch row that is read but was never written shows as NaN
    buf[:n].view(torch.float64).copy_(f.partial.reshape(-1))
    m_ref, is_ref, rm_ref, rv_ref = X.bn_stats_ref(f.S, f.Q, f.M, f.running_mean, f.running_var)
    for running in (True, False):
        mean, invstd = _nan(C), _nan(C)
        rm, rv = (f.running_mean.cuda(), f.running_var.cuda()) if running else (None, None)
        ops.bn_finalize(buf, tiles, f.M, C, mean, invstd, rm, rv)
        name = f"finalize {tiles} tiles x {C}, running={running}"
        assert_bitwise(mean, m_ref.float(), name + ": mean", 1.0 / f.M)
        assert_close_each(invstd, is_ref, 0.0, ULP2, name + ": invstd")
        if running:
            assert_bitwise(rm, rm_ref.float(), name + ": running_mean")
            assert_close_each(rv, rv_ref, 0.0, ULP2, name + ": running_var")


@functools.lru_cache(maxsize=None)
def _rows64(C):
    """The 64-row problem the apply pass of test_finalize_backward runs on (64 = 2^6: dgamma / M and dbeta / M are exact)."""
    return X.bn_rows_case(64, C, X.case_seed(64, C, 9))


@pytest.mark.parametrize("C,tiles", X.FINALIZE_CASES, ids=_ids)
def test_finalize_backward(ops, C, tiles):
    """mla_bn_bwd_from_partial on an fp32 [tiles][2][C] buffer of integers + its scratch tail: dbeta (slot 0) and dgamma (slot 1)
    bit-equal to the integer totals; the apply pass of the same call against the fp64 formula with the kernel's own dgamma / dbeta."""
    b = X.reduce_case("bwd_partials", tiles, C)
    r = _rows64(C)
    buf = torch.cat([b.partial.reshape(-1).cuda(), _nan(ops.bn_partial_scratch_elems(C))])
    mean, invstd, gamma, _ = _dev_channels(r.ch)
    dx, dgamma, dbeta = _nan(64, C), _nan(C), _nan(C)
    ops.bn_bwd_from_partial(r.g.cuda(), r.x.cuda(), mean, invstd, gamma, dx, dgamma, dbeta, buf, tiles, 64, C)
    name = f"backward finalize {tiles} tiles x {C}"
    assert_bitwise(dbeta, b.dbeta, name + ": dbeta", 1.0)
    assert_bitwise(dgamma, b.dgamma, name + ": dgamma", 1.0)
    assert_close_each(dx, X.bn_dx_rows(r.g, r.x, r.ch, dgamma.cpu(), dbeta.cpu(), 64), 1e-6, 2e-5, name + ": dx")


@pytest.mark.parametrize("C,tiles", X.FINALIZE_CASES, ids=_ids)
def test_finalize_order(ops, C, tiles):
    """The fp64 ORDER of the finalize regimes, which the integer cases above cannot see: on the cancelling partials of tests/exact.py
    (channel totals are rounding residue; test_reduce_exact_cpu.py proves that the regimes' orders and the sequential one give
    different bits there) the results are bit-equal to exact.order_total, the CPU restatement of the kernels' order of additions.
    Backward (mla_bn_bwd_from_partial, fp32 partials, apply pass on the 64-row problem): dbeta = float32(total of slot 0), dgamma =
    float32(total of slot 1).  Forward (mla_bn_finalize, fp64 partials): mean = float32(total of slot 0 / M).  invstd and the
    running statistics are not asserted here -- slot 1 cancels to noise and the variance clamps; test_finalize_forward holds them --
    but slot 1 of the double instantiation runs the same template code as slot 0, and the backward half covers slot 1 for the
    float instantiation."""
    c = X.reduce_case("cancelling", tiles, C)
    r = _rows64(C)
    name = f"finalize order ({X.finalize_regime(tiles)}) {tiles} tiles x {C}"

    want = X.order_total(c.bwd).float()
    buf = torch.cat([c.bwd.reshape(-1).cuda(), _nan(ops.bn_partial_scratch_elems(C))])
    mean, invstd, gamma, _ = _dev_channels(r.ch)
    dx, dgamma, dbeta = _nan(64, C), _nan(C), _nan(C)
    ops.bn_bwd_from_partial(r.g.cuda(), r.x.cuda(), mean, invstd, gamma, dx, dgamma, dbeta, buf, tiles, 64, C)
    assert_bitwise(dbeta, want[0], name + ": dbeta")
    assert_bitwise(dgamma, want[1], name + ": dgamma")
    assert not torch.isnan(dx).any(), name + ": dx"

    want = (X.order_total(c.fwd[:, 0]) / c.M).float()
    n = tiles * 2 * C * 2
    buf = _nan(n + ops.bn_partial_scratch_elems(C))
    buf[:n].view(torch.float64).copy_(c.fwd.reshape(-1))
    mean, invstd = _nan(C), _nan(C)
    ops.bn_finalize(buf, tiles, c.M, C, mean, invstd, None, None)
    assert_bitwise(mean, want, name + ": mean")
    assert not torch.isnan(invstd).any(), name + ": invstd"


# ---- 2. producer kernels: every legal C and the row edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", X.BN_ROW_CASES, ids=_ids)
def test_bn_rows(ops, M, C):
    """bn_stats_partial + bn_finalize, bn_apply, bn_bwd (with the ReLU mask + g_out, and in place without it) over [M][C] integer rows:
    the fp64 partial rows add up to exactly (sum x, sum x^2); dbeta / dgamma bit-equal to the exact sums; g_out the masked input bit for
    bit; the elementwise outputs against the fp64 formula."""
    c = X.reduce_case("bn_rows", M, C)
    name = f"[{M}][{C}]"
    xd, gd = c.x.cuda(), c.g.cuda()
    part = _nan(ops.bn_stats_partial_elems(M, C))
    tiles = ops.bn_stats_partial(xd, M, C, part)
    if M == 2 ** 18 + 1:
        assert tiles > 1024, "this case is meant to leave the one-launch finalize"
    rows = part[:tiles * 2 * C * 2].view(torch.float64).view(tiles, 2, C).cpu().sum(0)
    s, q = X.bn_stat_sums(c)
    assert_bitwise(rows[0], s.double(), name + " sum x", 1.0)
    assert_bitwise(rows[1], q.double(), name + " sum x^2", 1.0)
    mean, invstd = _nan(C), _nan(C)
    ops.bn_finalize(part, tiles, M, C, mean, invstd, None, None)
    m_ref, is_ref = X.bn_stats_ref(s, q, M)
    assert_bitwise(mean, m_ref.float(), name + " mean")                      # one correctly rounded fp64 divide, one rounding to fp32
    assert_close_each(invstd, is_ref, 0.0, ULP2, name + " invstd")

    # the elementwise passes run on the case's own exact statistics (integer mean, power-of-two invstd)
    mu, istd, gamma, beta = _dev_channels(c.ch)
    tail = slice(max(M - 4096, 0), M)
    out = _nan(M, C)
    ops.bn_apply(xd, mu, istd, gamma, beta, out, M, C, True, residual=c.res.cuda())
    out_ref = X.bn_apply_rows(c.x, c.ch, relu=True, residual=c.res)
    assert_close_each(out, out_ref, 1e-5, 1e-5, name + " bn_apply + residual + relu")
    out2 = _nan(M, C)
    ops.bn_apply(xd, mu, istd, gamma, beta, out2, M, C, False)
    assert_close_each(out2, X.bn_apply_rows(c.x, c.ch), 1e-5, 1e-5, name + " bn_apply")
    del out2

    mask = out_ref > 0
    gm = c.g * mask
    dg_ref, db_ref = X.bn_bwd_sums(c, mask)
    ws = _nan(ops.bn_bwd_ws_elems(M, C))
    dx, g_out, dgamma, dbeta = _nan(M, C), _nan(M, C), _nan(C), _nan(C)
    ops.bn_bwd(gd, xd, mu, istd, gamma, dx, dgamma, dbeta, ws, M, C, relu_out=out, g_out=g_out)
    assert_bitwise(dbeta, db_ref, name + " dbeta (masked)", X.G_UNIT)
    assert_bitwise(dgamma, dg_ref, name + " dgamma (masked)", X.G_UNIT / 8)
    assert_bitwise(g_out, gm, name + " g_out", X.G_UNIT)
    dx_ref = X.bn_dx_rows(gm, c.x, c.ch, dgamma.cpu(), dbeta.cpu(), M)
    assert_close_each(dx, dx_ref, 1e-6, 2e-5, name + " dx (masked)")
    assert_close_each(dx[tail], dx_ref[tail], 1e-6, 2e-5, name + " dx (masked), last rows")
    del dx, g_out, dx_ref

    dg_ref, db_ref = X.bn_bwd_sums(c)
    d2 = gd.clone()
    ws.fill_(NAN)
    ops.bn_bwd(d2, xd, mu, istd, gamma, d2, dgamma, dbeta, ws, M, C)               # in place: dx aliases dout
    assert_bitwise(dbeta, db_ref, name + " dbeta", X.G_UNIT)
    assert_bitwise(dgamma, dg_ref, name + " dgamma", X.G_UNIT / 8)
    dx_ref = X.bn_dx_rows(c.g, c.x, c.ch, dgamma.cpu(), dbeta.cpu(), M)
    assert_close_each(d2, dx_ref, 1e-6, 2e-5, name + " dx in place")
    assert_close_each(d2[tail], dx_ref[tail], 1e-6, 2e-5, name + " dx in place, last rows")
    assert_close_each(out[tail], out_ref[tail], 1e-5, 1e-5, name + " bn_apply, last rows")


# ---- 3. reductions fused into other kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math_", ["f32", "split"])
@pytest.mark.parametrize("geom,patch", X.DGRAD_BN_GEOMS, ids=_ids)
def test_dgrad_epilogue_reductions(ops, geom, patch, math_):
    """conv2d_dgrad / conv2d_dgrad_split with one and two BatchNorm requests on class D operands: dx is the exact integer map, and the
    per-tile sums the epilogue writes, finalized by bn_bwd_from_partial, give dgamma / dbeta bit-equal to the exact sums over it."""
    N, H, W, Cin, Cout, k, s, p = geom
    M = N * H * W
    c = X.reduce_case("dgrad_bn", geom)
    dyd, wd, resd, mskd = c.dy.cuda(), c.w.cuda(), c.res.cuda(), c.msk.cuda()
    zs = [z.cuda() for z in c.zs]
    chs = [_dev_channels(ch) for ch in c.chs]
    need = ops.conv2d_dgrad_bn_partial_elems(N, H, W, Cin)
    wS = ops.conv2d_wsplit(wd, False) if math_ == "split" else None
    wt_ws = torch.empty(wd.numel(), device="cuda")
    default = ops.conv2d_patch()
    if patch is not None and math_ == "split":      # the LDS-patch kernels exist on the split arithmetic only; for f32 this geometry is one
        ops.conv2d_patch(patch)                     # more gather-GEMM shape (49 row tiles of 128)
    try:
        for with_res, with_mask, nreq in ((True, True, 1), (True, True, 2), (False, True, 1), (False, False, 2)):
            v_ref = c.dx + c.res if with_res else c.dx.clone()
            if with_mask:
                v_ref = v_ref * (c.msk > 0)
            parts = [_nan(need) for _ in range(nreq)]
            kw = dict(dx=_nan(N, H, W, Cin), residual=resd if with_res else None, relu_src=mskd if with_mask else None,
                      bn_reqs=[(zs[q], chs[q][0], chs[q][1], parts[q]) for q in range(nreq)])
            if math_ == "split":
                dx, tiles = ops.conv2d_dgrad_split(dyd, wS, wd.shape, (N, H, W, Cin), s, p, **kw)
            else:
                dx, tiles = ops.conv2d_dgrad(dyd, wd, (N, H, W, Cin), s, p, wt_ws, **kw)
            name = f"{math_} dgrad {_ids(geom)} residual={with_res} mask={with_mask} requests={nreq}"
            assert_bitwise(dx, v_ref, name + ": dx", 1.0)
            if patch == 2 and math_ == "split":
                assert tiles == (M + 255) // 256, "the patch kernel did not run"
            for q in range(nreq):
                dg_ref, db_ref = X.dgrad_bn_sums(c, v_ref, q)
                o, dg, db = _nan(M, Cin), _nan(Cin), _nan(Cin)
                ops.bn_bwd_from_partial(dx.view(M, Cin), zs[q].view(M, Cin), chs[q][0], chs[q][1], chs[q][2], o, dg, db, parts[q], tiles, M, Cin)
                assert_bitwise(db, db_ref, f"{name}: dbeta (request {q})", 1.0)
                assert_bitwise(dg, dg_ref, f"{name}: dgamma (request {q})", 0.125)
                assert not torch.isnan(o).any()
    finally:
        ops.conv2d_patch(default)


@pytest.mark.parametrize("case", X.POOLED_CASES, ids=_ids)
def test_pooled_stem_backward(ops, case):
    """bn_bwd_pooled on integer data, with the decisions of bn_relu_maxpool_fwd: dgamma / dbeta bit-equal to the exact scatter-form sums;
    dy=None (the reduction half alone) gives the same bits."""
    N, H, W, C = case
    c = X.reduce_case("pooled", *case)
    yd, dpd = c.y.cuda(), c.dpool.cuda()
    mu, istd, gamma, beta = _dev_channels(c.ch)
    pooled, idx = _nan(N, c.OH, c.OW, C), torch.full((N, c.OH, c.OW, C), 255, device="cuda", dtype=torch.uint8)
    ops.bn_relu_maxpool_fwd(yd, mu, istd, gamma, beta, pooled, idx)
    dg_ref, db_ref, a_sel = X.pooled_sums(c, idx.cpu())
    name = f"pooled stem backward {_ids(case)}"
    assert_bitwise(pooled, a_sel.float(), name + ": pooled output vs the selected pixels")
    cpu_pool = torch.nn.functional.max_pool2d(c.act.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert_bitwise(pooled, cpu_pool.float(), name + ": pooled output vs the exact max-pool")
    M = N * H * W
    ws = _nan(ops.bn_bwd_ws_elems(M, C))
    dy, dg, db = _nan(N, H, W, C), _nan(C), _nan(C)
    ops.bn_bwd_pooled(dpd, idx, yd, mu, istd, gamma, beta, dy, dg, db, ws)
    assert_bitwise(db, db_ref, name + ": dbeta", 1.0)
    assert_bitwise(dg, dg_ref, name + ": dgamma", 0.125)
    # dy against the fp64 formula over the gather-form gradient g (|g| <= 4 * 7), r = g - a - b with a = dbeta / M, b = xhat * dgamma / M:
    # |a| <= 7 / 4 and |b| <= 4 * 7 (a quarter as many pooled outputs as pixels, |xhat| <= 4), at most five fp32 roundings of 2^-24 each
    # relative to a term, |gamma * invstd| <= 1: the absolute error stays below 5 * 2^-24 * (28 + 2 + 28) = 1.8e-5.  A misrouted window
    # moves a pixel by at least |gamma * invstd| >= 1/16.
    assert_close_each(dy, X.bn_dx_rows(X.pooled_gather(c, idx.cpu()), c.y, c.ch, dg.cpu(), db.cpu(), M), 2e-5, 0.0, name + ": dy")
    ws.fill_(NAN)
    dg2, db2 = _nan(C), _nan(C)
    ops.bn_bwd_pooled(dpd, idx, yd, mu, istd, gamma, beta, None, dg2, db2, ws)
    assert_bitwise(db2, db, name + ": dbeta, dy=None")
    assert_bitwise(dg2, dg, name + ": dgamma, dy=None")


# ---- 4. transformer column reductions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", X.COLSUM_CASES, ids=_ids)
def test_colsum_rows(ops, M, C):
    c = X.reduce_case("colsum", M, C)
    out, ws = _nan(C), _nan(ops.colreduce_ws_elems(M, C))
    ops.colsum_rows(c.x.cuda(), out, ws, M, C)
    assert_bitwise(out, c.total, f"colsum_rows [{M}][{C}]", 1.0)


@pytest.mark.parametrize("M,D", X.LN_CASES, ids=_ids)
def test_layernorm_bwd(ops, M, D):
    """layernorm_bwd on integer dy / x with fabricated integer mean[row] and power-of-two rstd[row]: db and dw bit-equal to sum dy and
    sum dy * xhat; dx without add, with add, and in place (dx aliases dy) against the fp64 formula at test_layernorm's tolerance."""
    c = X.reduce_case("ln", M, D)
    dyd, xd, wd, mud, rsd, addd = c.dy.cuda(), c.x.cuda(), c.w.cuda(), c.mean.cuda(), c.rstd.cuda(), c.add.cuda()
    n_ws = ops.colreduce_ws_elems(M, D)
    for variant in ("plain", "add", "in place + add"):
        dw, db, ws = _nan(D), _nan(D), _nan(n_ws)
        dx = dyd.clone() if variant.startswith("in place") else _nan(M, D)
        src = dx if variant.startswith("in place") else dyd
        ops.layernorm_bwd(src, xd, wd, mud, rsd, dx, dw, db, ws, M, D, add=None if variant == "plain" else addd)
        name = f"layernorm_bwd [{M}][{D}] {variant}"
        assert_bitwise(db, c.db, name + ": db", X.G_UNIT)
        assert_bitwise(dw, c.dw, name + ": dw", 2.0 ** -6)
        assert_close_each(dx, X.ln_dx_rows(c, None if variant == "plain" else c.add), 1e-5, 1e-5, name + ": dx")
