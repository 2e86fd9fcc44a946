"""The case tables of tests/pool_exact.py, proved on the CPU: a condition on the INPUTS of test_pool_exact_gpu.py.

Every budget holds; every code a geometry can have wins somewhere in it; the decision cases contain what their names claim; every
(H mod 4, W mod 4) pair and every (cgpb, nrl) layout is present; each first-trip case is past its cap by less than one trip and the
case below it is not; ATen's max-pool agrees with the tap-by-tap restatement of its rule, and the integer references with plain torch.
Then the wrappers of mla_hip.ops refuse wrong-sized outputs before any pointer reaches a kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact as X
import pool_exact as PX

_ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


def _same(a, b):
    """Bit-equal with NaN == NaN."""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) and \
        torch.equal(torch.isnan(a), torch.isnan(b))


def _check_maxpool(c):
    N, H, W, C = c.shape
    v, code = PX.window_rule(c.x)
    assert _same(v, c.y) and torch.equal(code, c.code), "ATen's max_pool2d and the tap-by-tap rule disagree"
    dx = PX.scatter_ref(c.dy_i, c.code, H, W)
    assert int(dx.abs().max()) <= 4 * 7
    # plain torch: autograd of max_pool2d routes the gradient to the same pixels (finite data; NaN / inf windows are the rule's alone)
    if torch.isfinite(c.x).all():
        xa = c.x.clone().requires_grad_(True)
        F.max_pool2d(xa.permute(0, 3, 1, 2), 3, 2, 1).backward(c.dy.permute(0, 3, 1, 2))
        assert torch.equal(xa.grad, dx.float()), "the int32 scatter and autograd disagree"
    assert torch.equal(dx.sum((1, 2)), c.dy_i.sum((1, 2), dtype=torch.int32)), "the scatter keeps every gradient exactly once"


def test_geometry_tables_hold_every_residue_and_code():
    assert {(H % 4, W % 4) for H, W in PX.GEOM_HW} == {(a, b) for a in range(4) for b in range(4)}
    assert {1, 2, 3} <= {H for H, _ in PX.GEOM_HW} and len(PX.GEOM_HW) == 81
    assert PX.possible_codes(1, 1) == [4] and PX.possible_codes(2, 2) == [4, 5, 7, 8] and PX.possible_codes(3, 3) == list(range(9))
    assert PX.possible_codes(1, 9) == [3, 4, 5] and PX.possible_codes(9, 1) == [1, 4, 7]
    for shape in PX.MAXPOOL_GEOM + PX.MAXPOOL_CHANNELS:
        c = PX.maxpool_case(shape)
        assert c.code.unique().tolist() == PX.possible_codes(shape[1], shape[2]), shape
        assert c.x.abs().max().item() <= 8 and torch.equal(c.x, c.x.round())
        _check_maxpool(c)
    for shape in PX.STEM_GEOM + PX.STEM_CHANNELS + list(PX.STEM_ROWS.values()):
        c = PX.stem_case(shape)
        idx = X.pooled_idx_cpu(c)
        assert idx.unique().tolist() == PX.possible_codes(shape[1], shape[2]), shape
        v, code = PX.window_rule(c.act.float())
        assert torch.equal(code, idx) and torch.equal(v.double(), X.pooled_sums(c, idx)[2])
    assert [s[3] for s in PX.STEM_CHANNELS] == [4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert {k: s[0] * PX.pool_out(s[1]) * PX.pool_out(s[2]) for k, s in PX.STEM_ROWS.items()} == {k: k for k in (31, 32, 33, 65)}
    assert all(PX.pool_out(s[1]) * PX.pool_out(s[2]) < 32 for s in PX.STEM_ROWS.values()), "a 32-row tile must span images"


@pytest.mark.parametrize("kind", PX.DECISIONS)
def test_decision_cases_contain_what_they_claim(kind):
    c = PX.decision_case(kind)
    N, H, W, C = c.shape
    _check_maxpool(c)
    OH, OW = c.y.shape[1], c.y.shape[2]
    oy, ox = torch.arange(OH).view(-1, 1), torch.arange(OW).view(1, -1)
    kh0, kw0 = (oy == 0).long(), (ox == 0).long()                    # the first valid tap of a window: 1 at the top / left edge
    first = (kh0 * 3 + kw0).view(1, OH, OW, 1).expand_as(c.code)
    kh1 = torch.clamp(H - 1 - (oy * 2 - 1), max=2)                   # the last valid one
    kw1 = torch.clamp(W - 1 - (ox * 2 - 1), max=2)
    last = (kh1 * 3 + kw1).view(1, OH, OW, 1).expand_as(c.code)
    # how often the maximum occurs in each window (finite cases)
    taps = F.unfold(F.pad(c.x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=-math.inf), 3, stride=2).view(N, C, 9, -1)
    if kind == "ties":
        fin = c.y.permute(0, 3, 1, 2).reshape(N, C, 1, -1)
        multi = ((taps == fin).sum(2) >= 2) & (fin[:, :, 0] != 0)
        assert multi.float().mean().item() > 0.1 and int(multi.sum()) >= 32, "ties between non-zero values must be common"
        assert set(c.code.unique().tolist()) == set(range(9))
    elif kind == "constant":
        assert (c.x == 3).all() and torch.equal(c.code.long(), first) and (c.y == 3).all()
    elif kind == "increasing":
        assert torch.equal(c.code.long(), last)
    elif kind == "decreasing":
        assert torch.equal(c.code.long(), first)
    elif kind == "neg_inf":
        assert (c.y == -math.inf).all() and torch.equal(c.code.long(), first)
    elif kind == "pos_inf_ties":
        n_inf = (taps == math.inf).sum(2)
        assert (n_inf >= 2).float().mean().item() > 0.3 and (n_inf == 0).any()
        assert (c.y[..., :] == math.inf).any() and torch.isfinite(c.y).any()
    elif kind == "nan_two":
        wy, wx = PX.NAN_WINDOW
        assert torch.isnan(c.y[:, wy, wx]).all() and (c.code[:, wy, wx] == 6).all(), "the later NaN takes the index"
        assert torch.isnan(taps).sum(2).max().item() == 2
    else:
        k = int(kind[-1])
        wy, wx = PX.NAN_WINDOW
        assert torch.isnan(c.y[:, wy, wx]).all() and (c.code[:, wy, wx] == k).all(), "a NaN wins and keeps its place"
        # a larger finite value follows the NaN in a window that holds both
        t = taps.permute(0, 1, 3, 2)
        nan_at = torch.isnan(t).float().argmax(-1)
        big_at = (t == 100).float().argmax(-1)
        both = torch.isnan(t).any(-1) & (t == 100).any(-1)
        assert (both & (big_at > nan_at)).any()
        assert torch.isnan(c.x).sum().item() == N * C
        # the windows with the NaN answer NaN, all others are finite
        assert torch.equal(torch.isnan(c.y.permute(0, 3, 1, 2).reshape(N, C, -1)), torch.isnan(t).any(-1))


def test_first_trip_cases_cross_their_caps_by_less_than_a_trip():
    cap = PX.POOL_CAP * PX.TPB
    f, b = PX.maxpool_units(PX.MAXPOOL_TRIP)
    assert f == 4210704 and cap < f < 2 * cap and PX.trips(f, PX.POOL_CAP) == 2 and PX.trips(b, PX.POOL_CAP) == 5
    assert PX.trips(PX.maxpool_units(PX.MAXPOOL_BELOW)[0], PX.POOL_CAP) == 1
    units = lambda s: math.prod(s[:2]) * s[2] // 4
    assert cap < units(PX.AVG_TRIP) < 2 * cap and PX.trips(units(PX.AVG_BELOW), PX.POOL_CAP) == 1
    assert max(math.prod(c) // 4 for c in PX.AVG_CASES) <= cap
    pixels = lambda s: s[0] * s[2] * s[3] * s[4]
    assert cap < pixels(PX.VIDEO_TRIP) < 2 * cap and PX.trips(pixels(PX.VIDEO_BELOW), PX.POOL_CAP) == 1
    assert PX.VIDEO_TRIP[1] == 3
    cap = PX.BN_EW_CAP * PX.TPB
    assert PX.stem_units(PX.STEM_FWD_TRIP)[0] == 2107392 and cap < 2107392 < 2 * cap
    assert PX.stem_units(PX.STEM_BWD_TRIP)[1] == 2107392
    assert PX.trips(PX.stem_units(PX.STEM_FWD_BELOW)[0], PX.BN_EW_CAP) == 1 and PX.trips(PX.stem_units(PX.STEM_BWD_BELOW)[1], PX.BN_EW_CAP) == 1
    # no other case of the tables reaches a second trip: the first-trip cases are the only ones that test it
    for s in PX.MAXPOOL_GEOM + PX.MAXPOOL_CHANNELS + [PX.DECISION_SHAPE]:
        assert max(PX.maxpool_units(s)) <= PX.POOL_CAP * PX.TPB
    for s in PX.STEM_GEOM + PX.STEM_CHANNELS + list(PX.STEM_ROWS.values()) + PX.STEM_WS:
        assert max(PX.stem_units(s)) <= cap


def test_workspace_cases_are_the_ones_the_old_tile_plan_overflowed():
    """At STEM_WS the tile rule applied to the pooled rows alone gives more partial rows than the workspace of M rows holds (the second
    one more than rows + scratch tail); at the workload's stem and at exact.POOLED_CASES it does not."""
    want = {(2341, 5, 7, 64): (878, 854), (10891, 1, 5, 64): (1022, 851)}
    for s in PX.STEM_WS:
        N, H, W, C = s
        MP = N * PX.pool_out(H) * PX.pool_out(W)
        assert (PX.ws_rows(MP), PX.ws_rows(N * H * W)) == want[s]
        X.assert_sum_budget(torch.tensor(MP * 7 * 8), f"pooled sums {s}")
    assert (1022 - 851) * 2 * 64 > 256 * 64 + 2
    for N, H, W, C in X.POOLED_CASES + [(192, 112, 112, 64), PX.STEM_BWD_TRIP]:
        assert PX.ws_rows(N * PX.pool_out(H) * PX.pool_out(W)) <= PX.ws_rows(N * H * W)
    assert PX.ws_rows(245760) == 1024 and PX.ws_rows(245761) == 961


def test_average_pool_cases():
    assert {PX.avg_layout(C)[:2] for C in PX.AVG_C} == {(4, 64), (8, 32), (16, 16), (32, 8), (64, 4), (128, 2), (256, 1)}
    assert {C: PX.avg_layout(C)[2] for C in (768, 2048)} == {768: 3, 2048: 2} and all(PX.avg_layout(C)[2] == 1 for C in PX.AVG_C if C not in (768, 2048))
    assert PX.avg_rows(1024) == [1, 2, 128, 147] and PX.avg_rows(16) == [1, 63, 64, 65, 128, 147]
    for NB, P, C in PX.AVG_CASES + [(3, 49, 64)]:
        c = PX.avg_case(NB, P, C)
        assert torch.equal(c.x.double().sum(1), c.S.double()) and torch.equal(c.x.flip(1).sum(1).double(), c.S.double())     # fp32 sums, two orders
        rel = ((c.fwd.double() - c.quot).abs() / c.quot.abs().clamp_min(1e-300))[c.S != 0]
        assert rel.numel() == 0 or rel.max().item() <= 2.0 ** -23, "the kernel's expression is within two roundings of S / P"
        assert (c.fwd[c.S == 0] == 0).all()
        if P & (P - 1) == 0:
            assert torch.equal(c.fwd.double(), c.quot)
        assert torch.equal(c.fwd, c.x.mean(1)) or P & (P - 1)          # plain torch agrees wherever the quotient is exact
        assert torch.allclose(c.fwd, c.x.mean(1), rtol=3e-7, atol=0)
        assert torch.equal(c.bwd_relu, c.bwd * (c.relu_src > 0)) and (c.relu_src == 0).any() and (c.dy != 0).all()


def test_layout_cases():
    assert [c[1] for c in PX.VIDEO_CASES] == [1, 3, 8, 1, 3, 8]
    for case in PX.VIDEO_CASES:
        src = PX.lane_image(case)
        B, C, T, H, W = case
        ref = PX.video_ref(src)
        assert ref.shape == (B * T, H, W, C) and ref[B * T - 1, H - 1, 0, C - 1] == src[B - 1, C - 1, T - 1, H - 1, 0]
    assert {(R, S) for _, R, S in PX.TRANSPOSE_CASES} == {(r, s) for r in PX.TRANSPOSE_SIZES for s in PX.TRANSPOSE_SIZES}
    assert all(math.prod(PX.split_hw(n)) == n for n in PX.TRANSPOSE_SIZES)
    img = PX.lane_image((3, 33, 70))
    assert img.unique().numel() == img.numel()


def test_stem_nan_and_forward_only_builders():
    c = PX.stem_nan_case()
    assert torch.isnan(c.y).sum().item() > 3 * 64 and torch.isnan(c.y[:, 4, 3]).all()
    v, code = PX.window_rule(c.act)
    av, acode = PX.aten_maxpool(c.act)
    assert torch.equal(code, acode) and torch.isnan(av).any() and torch.isfinite(av).any()
    # the lean fp32 builder of the first-trip forward case equals the fp64 one, on a small shape with the same channel count
    f = PX.stem_forward_only((2, 9, 7, 64))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    ref = X.bn_apply_rows(nhwc(f.y), f.ch, relu=True)
    assert torch.equal(nhwc(f.act).double(), ref)
    v, code = PX.window_rule(nhwc(f.act))
    assert torch.equal(v, nhwc(f.pooled)) and torch.equal(code, nhwc(f.code))


def test_stem_dy_bound_is_the_existing_one_at_the_existing_shapes():
    """At exact.POOLED_CASES' premises (|g| <= 28, |a| <= 2, |b| <= 28, |gamma * invstd| <= 1) the per-element bound never exceeds the 2e-5 of
    test_pooled_stem_backward."""
    assert 5 * 2.0 ** -24 * (28 + 2 + 28) < 2e-5
    c = PX.stem_case((3, 9, 7, 64))
    idx = X.pooled_idx_cpu(c)
    dg, db, _ = X.pooled_sums(c, idx)
    ref, tol = PX.stem_dy_bound(X.pooled_gather(c, idx), c.y, c.ch, dg, db, 3 * 9 * 7)
    assert torch.equal(ref, X.bn_dx_rows(X.pooled_gather(c, idx), c.y, c.ch, dg, db, 3 * 9 * 7))
    assert tol.max().item() < 5 * 2.0 ** -24 * (28 + 7 + 112)


# ---- the wrappers refuse before a pointer reaches a kernel -------------------------------------------------------------------------------
def test_wrappers_reject_wrong_shapes_before_launch():
    """CPU tensors: a shape refusal comes first (its message names the tensor); were the shapes accepted, _p would refuse the CPU tensor
    with another message -- which is what the rightly shaped calls at the end do."""
    from mla_hip import ops
    from mla_hip._lib import MLAHipError
    z = lambda *s: torch.zeros(s)
    b = lambda *s: torch.zeros(s, dtype=torch.uint8)
    ch = z(8)

    def refused(what, fn):
        with pytest.raises(MLAHipError, match=what):
            fn()

    x = z(2, 9, 7, 8)
    refused("maxpool_fwd: y has shape", lambda: ops.maxpool_fwd(x, z(2, 4, 4, 8), b(2, 5, 4, 8)))
    refused("maxpool_fwd: idx has shape", lambda: ops.maxpool_fwd(x, z(2, 5, 4, 8), b(2, 5, 4, 4)))
    refused("maxpool_fwd: x has shape", lambda: ops.maxpool_fwd(z(9, 7, 8), z(2, 5, 4, 8), b(2, 5, 4, 8)))
    refused("maxpool_bwd: dx has shape", lambda: ops.maxpool_bwd(z(2, 5, 4, 8), b(2, 5, 4, 8), z(2, 9, 6, 8), (2, 9, 7, 8)))
    refused("maxpool_bwd: dy has shape", lambda: ops.maxpool_bwd(z(2, 5, 3, 8), b(2, 5, 4, 8), x, (2, 9, 7, 8)))
    refused("maxpool_bwd: idx has shape", lambda: ops.maxpool_bwd(z(2, 5, 4, 8), b(2, 4, 4, 8), x, (2, 9, 7, 8)))
    refused("maxpool_bwd: relu_src has shape", lambda: ops.maxpool_bwd(z(2, 5, 4, 8), b(2, 5, 4, 8), x, (2, 9, 7, 8), relu_src=z(2, 9, 7, 4)))
    refused("maxpool_bwd: x_shape", lambda: ops.maxpool_bwd(z(2, 5, 4, 8), b(2, 5, 4, 8), x, (9, 7, 8)))
    refused("avgpool_fwd: y has 15 elements", lambda: ops.avgpool_fwd(z(3, 49, 16), z(15), 3, 49, 16))
    refused("avgpool_fwd: x has", lambda: ops.avgpool_fwd(z(3, 48, 16), z(3, 16), 3, 49, 16))
    refused("avgpool_bwd: dx has", lambda: ops.avgpool_bwd(z(3, 16), z(3, 48, 16), 3, 49, 16))
    refused("avgpool_bwd: dy has", lambda: ops.avgpool_bwd(z(2, 16), z(3, 49, 16), 3, 49, 16))
    refused("avgpool_bwd: relu_src has", lambda: ops.avgpool_bwd(z(3, 16), z(3, 49, 16), 3, 49, 16, relu_src=z(3, 49, 8)))
    refused("video_to_nhwc: dst has shape", lambda: ops.video_to_nhwc(z(2, 3, 3, 5, 7), z(6, 5, 7, 1)))
    refused("video_to_nhwc: src has shape", lambda: ops.video_to_nhwc(z(2, 3, 5, 7)))
    refused("nchw_to_nhwc: src has shape", lambda: ops.nchw_to_nhwc(z(3, 5, 7)))
    refused("nhwc_to_nchw: src has shape", lambda: ops.nhwc_to_nchw(z(3, 5, 7, 2, 2)))
    fwd = lambda **k: ops.bn_relu_maxpool_fwd(*[k.get(n, d) for n, d in (("y", x), ("mean", ch), ("invstd", ch), ("gamma", ch), ("beta", ch),
                                                                         ("out", z(2, 5, 4, 8)), ("idx", b(2, 5, 4, 8)))])
    refused("bn_relu_maxpool_fwd: out has shape", lambda: fwd(out=z(2, 5, 3, 8)))
    refused("bn_relu_maxpool_fwd: idx has shape", lambda: fwd(idx=b(1, 5, 4, 8)))
    refused("bn_relu_maxpool_fwd: gamma has shape", lambda: fwd(gamma=z(4)))
    refused("bn_relu_maxpool_fwd: y has shape", lambda: fwd(y=z(9, 7, 8)))
    need = ops.bn_bwd_ws_elems(2 * 9 * 7, 8)
    bwd = lambda **k: ops.bn_bwd_pooled(*[k.get(n, d) for n, d in (("dpool", z(2, 5, 4, 8)), ("idx", b(2, 5, 4, 8)), ("y", x), ("mean", ch), ("invstd", ch),
                                                                   ("gamma", ch), ("beta", ch), ("dy", z(2, 9, 7, 8)), ("dgamma", z(8)), ("dbeta", z(8)),
                                                                   ("ws", z(need)))])
    refused("bn_bwd_pooled: dy has shape", lambda: bwd(dy=z(2, 9, 7, 4)))
    refused("bn_bwd_pooled: dpool has shape", lambda: bwd(dpool=z(2, 4, 4, 8)))
    refused("bn_bwd_pooled: idx has shape", lambda: bwd(idx=b(2, 5, 4, 16)))
    refused("bn_bwd_pooled: dgamma has shape", lambda: bwd(dgamma=z(4)))
    refused("bn_bwd_pooled: dbeta has shape", lambda: bwd(dbeta=z(16)))
    refused("bn_bwd_pooled: ws has", lambda: bwd(ws=z(need - 1)))
    # rightly shaped CPU tensors pass the shape checks and are stopped at the pointer
    refused("expected a contiguous", lambda: ops.maxpool_fwd(x, z(2, 5, 4, 8), b(2, 5, 4, 8)))
    refused("expected a contiguous", lambda: ops.maxpool_bwd(z(2, 5, 4, 8), b(2, 5, 4, 8), z(2, 9, 7, 8), (2, 9, 7, 8)))
    refused("expected a contiguous", lambda: ops.avgpool_fwd(z(3, 49, 16), z(3, 16), 3, 49, 16))
    refused("expected a contiguous", lambda: ops.avgpool_bwd(z(3, 16), z(3, 49, 16), 3, 49, 16))
    refused("expected a contiguous", lambda: ops.video_to_nhwc(z(2, 3, 3, 5, 7), z(6, 5, 7, 3)))
    refused("expected a contiguous", lambda: fwd())
    refused("expected a contiguous", lambda: bwd())
    refused("expected a contiguous", lambda: bwd(dy=None))


def test_entry_points_refuse_bad_arguments_before_launch():
    """The C entry points with never-dereferenced pointers: every refusal the host half makes is reached through the library too."""
    from mla_hip import _lib
    lib = _lib.load()
    q = 0x1000
    err = lambda: lib.mla_last_error()
    assert lib.mla_maxpool3x3s2_fwd(q, q, q, 2, 9, 7, 6, None) == -1 and b"mla_maxpool3x3s2_fwd: bad argument" in err()
    assert lib.mla_maxpool3x3s2_bwd(q, q, None, None, 2, 9, 7, 8, None) == -1 and b"mla_maxpool3x3s2_bwd: bad argument" in err()
    for C in (4, 8, 12, 24):
        assert lib.mla_avgpool_fwd(q, q, 3, 49, C, None) == -1 and b"unsupported" in err()
    assert lib.mla_avgpool_fwd(q, q, 3, 49, 18, None) == -1 and b"mla_avgpool_fwd: bad argument" in err()
    assert lib.mla_avgpool_bwd(q, None, None, 3, 49, 16, None) == -1 and b"mla_avgpool_bwd: bad argument" in err()
    assert lib.mla_video_to_nhwc(q, q, 2, 9, 3, 5, 7, None) == -1 and b"mla_video_to_nhwc: bad argument" in err()
    assert lib.mla_nchw_to_nhwc(q, q, 65536, 3, 5, 7, None) == -1 and b"transpose: bad argument" in err()
    assert lib.mla_nhwc_to_nchw(q, None, 3, 3, 5, 7, None) == -1 and b"transpose: bad argument" in err()
    assert lib.mla_bn_relu_maxpool_fwd(q, q, q, q, q, q, q, 2, 9, 7, 12, None) == -1 and b"must be 4*2^k" in err()
    assert lib.mla_bn_relu_maxpool_fwd(q, q, q, q, q, None, q, 2, 9, 7, 8, None) == -1 and b"mla_bn_relu_maxpool_fwd: bad argument" in err()
    assert lib.mla_bn_bwd_pooled(q, q, q, q, q, q, q, q, q, q, None, 2, 9, 7, 8, None) == -1 and b"mla_bn_bwd_pooled: null pointer" in err()
    assert lib.mla_bn_bwd_pooled(q, q, q, q, q, q, q, q, q, q, q, 65536, 256, 128, 8, None) == -1 and b"mla_bn_bwd_pooled: bad dims" in err()
    assert lib.mla_bn_bwd_pooled(q, q, q, q, q, q, q, q, q, q, q, 2, 9, 7, 12, None) == -1 and b"must be 4*2^k" in err()
