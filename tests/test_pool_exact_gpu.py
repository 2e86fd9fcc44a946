"""The pooling and layout kernels (csrc/pool.hip) and the two stem kernels that fuse BatchNorm into the max-pool (csrc/bn.hip) at every
window class, channel regime and grid trip, against exact references (tests/pool_exact.py; test_pool_exact_cpu.py proves the tables).

  max-pool       values and codes bit-equal to ATen on the CPU at every (H, W) in 1..9, on ties between non-zero values, constant and
                 monotone images, -inf, +inf ties and NaN at every tap; the backward bit-equal to the integer scatter, with and
                 without the ReLU source; the first case whose grids wrap their grid-stride loops.
  average pool   every (cgpb, nrl) layout, fewer rows than row lanes, grid.y > 1: bit-equal to fp32(S) * fp32(1 / P) with the exact
                 integer sum S, within 2^-23 of S / P, bit-equal to S / P for P a power of two; the backward past its capped grid.
  layout         torch.equal with the permuted tensor, either side of the 32 x 32 tile, past the capped grid.
  fused stem     the forward bit-equal to ATen and to bn_apply -> maxpool_fwd; dgamma / dbeta bit-equal to the int64 sums at every
                 admitted C and every (H mod 4, W mod 4); the two shapes whose partial rows used to outgrow the workspace; both
                 capped grids past their first trip.

Every output lives between sentinels, every input between NaN, the workspace is sized exactly by bn_bwd_ws_elems.  Every launch runs
twice, into an interior of NaN and into one of a finite filler: the two results must be bit-identical -- so every element was written
and nothing depends on what the buffer held -- and the sentinels intact.  No case is skipped or relaxed."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import exact as X  # noqa: E402
import pool_exact as PX  # noqa: E402

GUARD = 1024                  # elements on either side of every buffer (a multiple of 16: float4 and uchar4 views stay aligned)
SENTINEL, FILLER = -12345.5, -777.25
IDX_SENTINEL, IDX_FILLERS = 0xA5, (255, 99)            # no code (0..8) equals any of them
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


class Out:
    """An output buffer: SENTINEL on either side of an interior of `shape`, filled with NaN (run 0) or FILLER (run 1); uint8 alike."""

    def __init__(self, shape, run, dtype=torch.float32):
        self.u8 = dtype == torch.uint8
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), IDX_SENTINEL if self.u8 else SENTINEL, device="cuda", dtype=dtype)
        self.v = self.buf[GUARD:GUARD + n].view(shape)
        self.v.fill_(IDX_FILLERS[run] if self.u8 else (NAN, FILLER)[run])

    def intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        return bool((g == (IDX_SENTINEL if self.u8 else SENTINEL)).all())


def inp(src, dtype=torch.float32):
    """An input: a contiguous device view of src with NaN (255 for index bytes) around it."""
    src = src.to(dtype)
    buf = torch.full((src.numel() + 2 * GUARD,), 255 if dtype == torch.uint8 else NAN, device="cuda", dtype=dtype)
    v = buf[GUARD:GUARD + src.numel()].view(src.shape)
    v.copy_(src)
    return v


def same(a, b):
    """Bit-equal, NaN equal to NaN (the payload of a NaN is not part of any contract here)."""
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    an, bn = torch.isnan(a), torch.isnan(b)
    return torch.equal(an, bn) and torch.equal(torch.where(an, torch.zeros_like(a), a), torch.where(bn, torch.zeros_like(b), b))


def assert_same(got, want, name):
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if same(got, want):
        return
    both_nan = torch.isnan(got) & torch.isnan(want) if got.dtype.is_floating_point else torch.zeros_like(got, dtype=torch.bool)
    bad = ~((got == want) | both_nan)
    first = torch.nonzero(bad)[0].tolist()
    raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at index {first}: got {got[tuple(first)].item()!r}, "
                         f"want {want[tuple(first)].item()!r}")


def twice(name, launch, specs, may_nan=False, scratch=()):
    """launch(*views) into fresh guarded outputs of specs = [(shape, dtype)], once over NaN and once over FILLER; returns the views of
    the first run after holding the second to the same bits and both to their sentinels.  may_nan: the reference has NaN too;
    scratch: indices of workspaces, which need not be written everywhere -- only their sentinels are looked at."""
    runs = []
    for run in (0, 1):
        outs = [Out(shape, run, dtype) for shape, dtype in specs]
        launch(*[o.v for o in outs])
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert o.intact(), f"{name}: a store left output {k}"
        runs.append([o.v for o in outs])
    for k, (a, b) in enumerate(zip(*runs)):
        if k in scratch:
            continue
        assert same(a, b), f"{name}: output {k} depends on what the buffer held (an element was not written), or two runs differ"
        if a.dtype == torch.uint8:
            assert int(a.max()) <= 8, f"{name}: output {k} holds a byte that is no code"
        elif not may_nan:
            assert not torch.isnan(a).any(), f"{name}: output {k} holds NaN (an element was not written, or a read left an input)"
    return runs[0]


F32, U8 = torch.float32, torch.uint8


# ---- max-pool --------------------------------------------------------------------------------------------------------------------------
def run_maxpool(ops, c, name, may_nan=False):
    """Forward against ATen's values and codes; backward, fed with the reference's codes, against the integer scatter with and without
    the ReLU source."""
    N, H, W, C = c.shape
    xd = inp(c.x)
    y, idx = twice(name + " fwd", lambda y, i: ops.maxpool_fwd(xd, y, i), [(c.y.shape, F32), (c.y.shape, U8)], may_nan)
    assert_same(y, c.y, name + ": maxima vs ATen")
    assert_same(idx, c.code, name + ": codes vs ATen")
    dyd, coded, rd = inp(c.dy), inp(c.code, U8), inp(c.relu_src)
    dx_ref = PX.scatter_ref(c.dy_i, c.code, H, W).float()
    dx, = twice(name + " bwd", lambda dx: ops.maxpool_bwd(dyd, coded, dx, c.shape), [(c.shape, F32)])
    assert_same(dx, dx_ref, name + ": backward vs the integer scatter")
    dx, = twice(name + " bwd relu", lambda dx: ops.maxpool_bwd(dyd, coded, dx, c.shape, relu_src=rd), [(c.shape, F32)])
    assert_same(dx, dx_ref * (c.relu_src > 0), name + ": backward under the ReLU source")


@pytest.mark.parametrize("table", ["geometry", "channels"])
def test_maxpool_every_window_class(ops, table):
    """Every (H, W) in 1..9 squared at N = 2, C = 8 (H or W of 1, 2, 3: windows that are all edge); C = 4 .. 512 at 3 x 9 x 7."""
    for shape in (PX.MAXPOOL_GEOM if table == "geometry" else PX.MAXPOOL_CHANNELS):
        run_maxpool(ops, PX.maxpool_case(shape), f"maxpool {_ids(shape)}")


@pytest.mark.parametrize("kind", PX.DECISIONS)
def test_maxpool_decisions(ops, kind):
    """First maximum in row-major order, `val > max || isnan(val)`: ties, constant, monotone, infinities, NaN at each tap, two NaN."""
    run_maxpool(ops, PX.decision_case(kind), f"maxpool {kind}", may_nan=kind.startswith("nan"))


def test_maxpool_past_the_grid_cap(ops):
    """(1, 1025, 1025, 64): the forward is 16 400 float4 past its 16384-workgroup grid, the backward loops five times.  The CPU side is
    ATen's max-pool and an fp32 scatter (integers below 2^24: exact); the comparison runs on the device, over every element."""
    shape = PX.MAXPOOL_TRIP
    c = PX.maxpool_case(shape)
    N, H, W, C = shape
    xd = inp(c.x)
    y, idx = twice("maxpool trip fwd", lambda y, i: ops.maxpool_fwd(xd, y, i), [(c.y.shape, F32), (c.y.shape, U8)])
    assert_same(y, c.y, "maxpool past the cap: maxima")
    assert_same(idx, c.code, "maxpool past the cap: codes")
    dx_ref = PX.scatter_ref(c.dy_i, c.code, H, W, dtype=torch.float32).cuda()
    dyd, coded, rd = inp(c.dy), inp(c.code, U8), inp(c.relu_src)
    del xd, y, idx
    dx, = twice("maxpool trip bwd", lambda dx: ops.maxpool_bwd(dyd, coded, dx, shape), [(shape, F32)])
    assert_same(dx, dx_ref, "maxpool past the cap: backward")
    del dx
    dx, = twice("maxpool trip bwd relu", lambda dx: ops.maxpool_bwd(dyd, coded, dx, shape, relu_src=rd), [(shape, F32)])
    assert_same(dx, dx_ref * (rd > 0), "maxpool past the cap: backward under the ReLU source")


# ---- average pool ----------------------------------------------------------------------------------------------------------------------
def run_avgpool(ops, case, name):
    NB, P, C = case
    c = PX.avg_case(*case)
    xd, dyd, rd = inp(c.x), inp(c.dy), inp(c.relu_src)
    y, = twice(name + " fwd", lambda y: ops.avgpool_fwd(xd, y, NB, P, C), [((NB, C), F32)])
    assert_same(y, c.fwd, name + ": vs fp32(S) * fp32(1 / P)")
    rel = ((y.double().cpu() - c.quot).abs() / c.quot.abs().clamp_min(1e-300))[c.S != 0]
    worst = rel.max().item() if rel.numel() else 0.0
    print(f"{name}: worst relative error vs S / P = {worst:.3g} (bound 2^-23 = {2.0 ** -23:.3g})")
    assert worst <= 2.0 ** -23 and bool((y.cpu()[c.S == 0] == 0).all())
    if P & (P - 1) == 0:
        assert_same(y.double(), c.quot, name + ": P a power of two, the mean itself")
    dx, = twice(name + " bwd", lambda dx: ops.avgpool_bwd(dyd, dx, NB, P, C), [((NB, P, C), F32)])
    assert_same(dx, c.bwd, name + ": backward")
    dx, = twice(name + " bwd relu", lambda dx: ops.avgpool_bwd(dyd, dx, NB, P, C, relu_src=rd), [((NB, P, C), F32)])
    assert_same(dx, c.bwd_relu, name + ": backward under the ReLU source")


@pytest.mark.parametrize("C", PX.AVG_C)
def test_avgpool_every_layout(ops, C):
    """One channel count = one (cgpb, nrl) layout (768 and 2048: grid.y > 1): P = 1, either side of the number of row lanes, 128, 147;
    one and three images."""
    for case in [k for k in PX.AVG_CASES if k[2] == C]:
        run_avgpool(ops, case, f"avgpool {_ids(case)}")


def test_avgpool_past_the_grid_cap(ops):
    """(33, 1024, 512): the backward is 131 072 float4 past its 16384-workgroup grid."""
    run_avgpool(ops, PX.AVG_TRIP, f"avgpool {_ids(PX.AVG_TRIP)}")


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
def run_video(ops, case):
    B, C, T, H, W = case
    src = PX.lane_image(case)
    sd = inp(src)
    dst, = twice(f"video_to_nhwc {_ids(case)}", lambda d: ops.video_to_nhwc(sd, d), [((B * T, H, W, C), F32)])
    assert torch.equal(dst, PX.video_ref(src).cuda()), f"video_to_nhwc {_ids(case)}"


def test_video_to_nhwc(ops):
    for case in PX.VIDEO_CASES:
        run_video(ops, case)


def test_video_to_nhwc_past_the_grid_cap(ops):
    """28 clips of 3 frames of 224 x 224: 20 480 pixels past the 16384-workgroup grid."""
    run_video(ops, PX.VIDEO_TRIP)


def test_transposes(ops):
    """[R][S] -> [S][R] per image for R, S either side of the 32 x 32 tile, three images, through both entry points, which differ in
    which of the two sizes is the channel count."""
    for n, R, S in PX.TRANSPOSE_CASES:
        src = PX.lane_image((n, R, S))
        sd, want = inp(src), src.transpose(1, 2).contiguous().cuda()
        h, w = PX.split_hw(S)
        dst, = twice(f"nchw_to_nhwc {R}x{S}", lambda d: ops._call("mla_nchw_to_nhwc", ops._p(sd), ops._p(d), n, R, h, w, ops.cur_stream()),
                     [((n, S, R), F32)])
        assert torch.equal(dst, want), f"nchw_to_nhwc C={R} HW={S}"
        h, w = PX.split_hw(R)
        dst, = twice(f"nhwc_to_nchw {R}x{S}", lambda d: ops._call("mla_nhwc_to_nchw", ops._p(sd), ops._p(d), n, S, h, w, ops.cur_stream()),
                     [((n, S, R), F32)])
        assert torch.equal(dst, want), f"nhwc_to_nchw HW={R} C={S}"
        assert torch.equal(ops.nchw_to_nhwc(sd.view(n, R, *PX.split_hw(S))).view(n, S, R), want)          # the allocating wrappers
        assert torch.equal(ops.nhwc_to_nchw(sd.view(n, *PX.split_hw(R), S)).view(n, S, R), want)


# ---- fused stem ------------------------------------------------------------------------------------------------------------------------
def _channels(ch):
    return [inp(t) for t in (ch.mean, ch.invstd, ch.gamma, ch.beta)]


def run_stem_forward(ops, yd, chd, shape, name, may_nan=False):
    """bn_relu_maxpool_fwd and the two-kernel path bn_apply -> maxpool_fwd: the same bits.  Returns (pooled, idx) of the fused kernel."""
    N, H, W, C = shape
    ps = (N, PX.pool_out(H), PX.pool_out(W), C)
    pooled, idx = twice(name + " fused fwd", lambda o, i: ops.bn_relu_maxpool_fwd(yd, *chd, o, i), [(ps, F32), (ps, U8)], may_nan)
    act, = twice(name + " bn_apply", lambda a: ops.bn_apply(yd, *chd, a, N * H * W, C, True), [(shape, F32)], may_nan)
    p2, i2 = twice(name + " maxpool_fwd", lambda o, i: ops.maxpool_fwd(act, o, i), [(ps, F32), (ps, U8)], may_nan)
    assert_same(pooled, p2, name + ": fused maxima vs bn_apply -> maxpool_fwd")
    assert_same(idx, i2, name + ": fused codes vs bn_apply -> maxpool_fwd")
    return pooled, idx


def run_stem(ops, shape, name):
    """Forward against ATen; backward with the exact workspace: dgamma / dbeta bit-equal to the int64 scatter-form sums (dy=None: the same
    bits), dy element by element at the bound of pool_exact.stem_dy_bound."""
    N, H, W, C = shape
    c = PX.stem_case(shape)
    M = N * H * W
    yd, chd = inp(c.y), _channels(c.ch)
    pooled, idx = run_stem_forward(ops, yd, chd, shape, name)
    aten_v, aten_code = PX.aten_maxpool(c.act.float())
    assert_same(pooled, aten_v, name + ": maxima vs ATen")
    assert_same(idx, aten_code, name + ": codes vs ATen")
    dg_ref, db_ref, _ = X.pooled_sums(c, aten_code)
    dpd, idxd = inp(c.dpool), inp(aten_code, U8)
    n_ws = ops.bn_bwd_ws_elems(M, C)
    dy, dg, db, _ = twice(name + " bwd", lambda dy, dg, db, ws: ops.bn_bwd_pooled(dpd, idxd, yd, *chd, dy, dg, db, ws),
                          [(shape, F32), ((C,), F32), ((C,), F32), ((n_ws,), F32)], scratch=(3,))
    X.assert_bitwise(db, db_ref, name + ": dbeta", 1.0)
    X.assert_bitwise(dg, dg_ref, name + ": dgamma", 0.125)
    dg2, db2, _ = twice(name + " bwd, dy=None", lambda dg, db, ws: ops.bn_bwd_pooled(dpd, idxd, yd, *chd, None, dg, db, ws),
                        [((C,), F32), ((C,), F32), ((n_ws,), F32)], scratch=(2,))
    X.assert_bitwise(db2, db_ref, name + ": dbeta, dy=None")
    X.assert_bitwise(dg2, dg_ref, name + ": dgamma, dy=None")
    dy = dy.cpu()
    worst, step = 0.0, max(1, (1 << 22) // (H * W * C))                     # images per chunk: the fp64 temporaries stay small
    for n0 in range(0, N, step):
        s = slice(n0, n0 + step)
        part = SimpleNamespace(N=len(range(N)[s]), H=H, W=W, C=C, OH=c.OH, OW=c.OW, act=c.act[s], dpool=c.dpool[s])
        ref, tol = PX.stem_dy_bound(X.pooled_gather(part, aten_code[s]), c.y[s], c.ch, dg_ref, db_ref, M)
        err = (dy[s].double() - ref).abs()
        assert bool((err <= tol).all()), f"{name}: dy, images {n0}..: {int((err > tol).sum())} elements outside 5 * 2^-24 * (|g| + |a| + |b|)"
        worst = max(worst, (err / tol.clamp_min(1e-300)).max().item())
    print(f"{name}: dy worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("table", ["geometry", "rows"])
def test_stem_every_window_class(ops, table):
    """Every (H, W) in 1..9 squared at N = 2, C = 8: every (H mod 4, W mod 4) of the 2x2-block forward and the 2x2-quad backward; 31, 32,
    33 and 65 pooled rows at C = 64: either side of the 32-row tile, tiles that span images."""
    for shape in (PX.STEM_GEOM if table == "geometry" else list(PX.STEM_ROWS.values())):
        run_stem(ops, shape, f"stem {_ids(shape)}")


@pytest.mark.parametrize("C", PX.STEM_C)
def test_stem_every_channel_count(ops, C):
    """Every C = 4 * 2^k <= 1024: nrl = 256 / (C / 4) row lanes in the pooled reduction, from 256 down to 1."""
    run_stem(ops, (3, 9, 7, C), f"stem 3x9x7x{C}")


def test_stem_forward_nan(ops):
    """NaN in y: it passes BatchNorm and the ReLU, wins its windows and keeps its place -- in the fused kernel and in bn_apply ->
    maxpool_fwd alike."""
    c = PX.stem_nan_case()
    pooled, idx = run_stem_forward(ops, inp(c.y), _channels(c.ch), (c.N, c.H, c.W, c.C), "stem NaN", may_nan=True)
    aten_v, aten_code = PX.aten_maxpool(c.act)
    assert torch.isnan(aten_v).any()
    assert_same(pooled, aten_v, "stem NaN: maxima vs ATen")
    assert_same(idx, aten_code, "stem NaN: codes vs ATen")


@pytest.mark.parametrize("shape", PX.STEM_WS, ids=_ids)
def test_stem_backward_fits_its_workspace(ops, shape):
    """The shapes at which the tile rule of the pooled rows alone asked for more partial rows than bn_bwd_ws_elems(N * H * W, C) holds
    (878 of 854; 1022 of 851, past the scratch tail too): the workspace is exactly that size, between sentinels."""
    run_stem(ops, shape, f"stem {_ids(shape)}")


def test_stem_forward_past_the_grid_cap(ops):
    """(168, 112, 112, 64): 10 240 thread quads past the 8192-workgroup grid.  y, relu(bn(y)) and ATen's max-pool are formed in fp32
    on the CPU (exact on these data) in NCHW; the permutation and the comparison of every element run on the device."""
    shape = PX.STEM_FWD_TRIP
    f = PX.stem_forward_only(shape)
    nhwc = lambda t: t.cuda().permute(0, 2, 3, 1).contiguous()
    want_v, want_code = nhwc(f.pooled), nhwc(f.code)
    yd, chd = inp(nhwc(f.y)), _channels(f.ch)
    N, H, W, C = shape
    ps = tuple(want_v.shape)
    pooled, idx = twice("stem trip fwd", lambda o, i: ops.bn_relu_maxpool_fwd(yd, *chd, o, i), [(ps, F32), (ps, U8)])
    assert_same(pooled, want_v, "stem forward past the cap: maxima vs ATen")
    assert_same(idx, want_code, "stem forward past the cap: codes vs ATen")
    act = torch.empty(shape, device="cuda")
    ops.bn_apply(yd, *chd, act, N * H * W, C, True)
    assert_same(act, nhwc(f.act), "bn_apply (its own second trip)")
    p2, i2 = twice("stem trip maxpool_fwd", lambda o, i: ops.maxpool_fwd(act, o, i), [(ps, F32), (ps, U8)])
    assert_same(pooled, p2, "stem forward past the cap: fused maxima vs bn_apply -> maxpool_fwd")
    assert_same(idx, i2, "stem forward past the cap: fused codes vs bn_apply -> maxpool_fwd")


def test_stem_backward_past_the_grid_cap(ops):
    """(42, 112, 112, 64): the apply pass is 10 240 pixel quads past the 8192-workgroup grid."""
    run_stem(ops, PX.STEM_BWD_TRIP, f"stem {_ids(PX.STEM_BWD_TRIP)}")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ops):
    """What the host half refuses raises MLAHipError, and no output is touched: C % 4 != 0, the avgpool's C in {4, 8, 12, 24}, a video of 9
    channels, 65536 images to transpose, null pointers, channel counts the BatchNorm family does not take, wrong-sized outputs."""
    from mla_hip._lib import MLAHipError
    z = lambda *s: torch.zeros(s, device="cuda")
    outs = []

    def out(shape, dtype=F32):
        outs.append(Out(shape, 0, dtype))
        return outs[-1].v

    def refused(fn):
        with pytest.raises(MLAHipError):
            fn()

    refused(lambda: ops.maxpool_fwd(z(2, 9, 7, 6), out((2, 5, 4, 6)), out((2, 5, 4, 6), U8)))
    refused(lambda: ops.maxpool_bwd(z(2, 5, 4, 6), torch.zeros((2, 5, 4, 6), device="cuda", dtype=U8), out((2, 9, 7, 6)), (2, 9, 7, 6)))
    refused(lambda: ops.maxpool_fwd(z(2, 9, 7, 8), out((2, 5, 4, 8)), None))
    refused(lambda: ops.maxpool_fwd(z(2, 9, 7, 8), out((2, 4, 4, 8)), out((2, 5, 4, 8), U8)))
    for C in (4, 8, 12, 24, 18):
        refused(lambda: ops.avgpool_fwd(z(3, 49, C), out((3, C)), 3, 49, C))
    refused(lambda: ops.avgpool_fwd(None, out((3, 16)), 3, 49, 16))
    refused(lambda: ops.avgpool_fwd(z(3, 49, 16), out((2, 16)), 3, 49, 16))
    refused(lambda: ops.avgpool_bwd(z(3, 18), out((3, 49, 18)), 3, 49, 18))
    refused(lambda: ops.avgpool_bwd(None, out((3, 49, 16)), 3, 49, 16))
    refused(lambda: ops.avgpool_bwd(z(3, 16), out((3, 48, 16)), 3, 49, 16))
    refused(lambda: ops.video_to_nhwc(z(2, 9, 3, 5, 7), out((6, 5, 7, 9))))
    refused(lambda: ops.video_to_nhwc(z(2, 3, 3, 5, 7), out((6, 5, 7, 1))))
    big = z(65536, 1, 1, 2)
    refused(lambda: ops._call("mla_nchw_to_nhwc", ops._p(big), ops._p(out((65536, 2))), 65536, 1, 1, 2, ops.cur_stream()))
    refused(lambda: ops._call("mla_nhwc_to_nchw", ops._p(big), ops._p(out((65536, 2))), 65536, 2, 1, 1, ops.cur_stream()))
    refused(lambda: ops._call("mla_nchw_to_nhwc", None, ops._p(out((3, 2))), 3, 1, 1, 2, ops.cur_stream()))
    ch12, ch8 = [z(12)] * 4, [z(8)] * 4
    refused(lambda: ops.bn_relu_maxpool_fwd(z(2, 9, 7, 12), *ch12, out((2, 5, 4, 12)), out((2, 5, 4, 12), U8)))
    refused(lambda: ops.bn_relu_maxpool_fwd(z(2, 9, 7, 8), *ch8, out((2, 5, 4, 8)), None))
    refused(lambda: ops.bn_relu_maxpool_fwd(z(2, 9, 7, 8), *ch8, out((2, 5, 3, 8)), out((2, 5, 4, 8), U8)))
    i8 = torch.zeros((2, 5, 4, 8), device="cuda", dtype=U8)
    n_ws = ops.bn_bwd_ws_elems(2 * 9 * 7, 8)
    refused(lambda: ops.bn_bwd_pooled(z(2, 5, 4, 12), torch.zeros((2, 5, 4, 12), device="cuda", dtype=U8), z(2, 9, 7, 12), *ch12, out((2, 9, 7, 12)),
                                      out((12,)), out((12,)), out((ops.bn_bwd_ws_elems(126, 12),))))
    refused(lambda: ops.bn_bwd_pooled(z(2, 5, 4, 8), i8, z(2, 9, 7, 8), *ch8, out((2, 9, 7, 8)), out((8,)), None, out((n_ws,))))
    refused(lambda: ops.bn_bwd_pooled(z(2, 5, 4, 8), i8, z(2, 9, 7, 8), *ch8, out((2, 9, 7, 8)), out((8,)), out((8,)), out((n_ws - 1,))))
    refused(lambda: ops.bn_bwd_pooled(z(2, 5, 4, 8), i8, z(2, 9, 7, 8), *ch8, out((2, 9, 6, 8)), out((8,)), out((8,)), out((n_ws,))))
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert o.intact(), f"refused call: a store left output {k}"
        untouched = (o.v == IDX_FILLERS[0]).all() if o.u8 else torch.isnan(o.v).all()
        assert bool(untouched), f"refused call: output {k} was written"
