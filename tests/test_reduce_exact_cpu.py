"""The exactly-summable inputs of the reduction tests (tests/exact.py, second half), checked on the CPU: a condition on the INPUTS of
test_reduce_exact_gpu.py.

For every builder and every case that file runs: the 2^24 budget holds (the builders assert it, no case is skipped or relaxed), the
int64 reference equals an fp64 evaluation of the same sums (in fp32 too, in more than one order, where that is cheap), the tile
contributions are non-zero and distinct, and the two slots of a partial row have different totals -- so that a dropped, doubled or
swapped tile, row or slot moves a result by at least one unit.

For the order pin (test_finalize_order): the vectorised restatement of the kernels' summation order equals a tile-by-tile loop, and
the cancelling partials give different bits for every pair of orders."""
import pytest
import torch

import exact as X

_ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


@pytest.mark.parametrize("C,tiles", X.FINALIZE_CASES, ids=_ids)
def test_fabricated_partials(C, tiles):
    f = X.reduce_case("fwd_partials", tiles, C)
    assert f.M & (f.M - 1) == 0 and 32 * tiles <= f.M < 64 * tiles
    perm = torch.randperm(tiles, generator=torch.Generator().manual_seed(tiles))
    for order in (f.partial, f.partial[perm]):
        tot = order.sum(0)
        assert torch.equal(tot[0], f.S.double()) and torch.equal(tot[1], f.Q.double()), "fp64 sums of the forward partials"
    mean, invstd, rm, rv = X.bn_stats_ref(f.S, f.Q, f.M, f.running_mean, f.running_var)
    assert torch.equal(mean.float().double(), mean), "s / M must be exact in fp32"
    var = f.Q.double() / f.M - mean * mean
    assert var.min().item() > 7.0 and mean.abs().max().item() <= 3.0, "the variance must stay well away from cancellation"
    u, unit = X.running_units(f.S, f.rm4, f.M)
    assert torch.equal(u.double() * unit, rm), "running_mean: the fp64 evaluation is the exact value"
    assert torch.isfinite(invstd).all() and torch.isfinite(rv).all()
    # dropping any one tile moves sum x by at least 1 (and sum x^2 by at least 1024) in every channel
    assert (f.ints[:, 0] != 0).all() and (f.ints[:, 1] >= 1024).all()

    b = X.reduce_case("bwd_partials", tiles, C)
    for order in (b.partial, b.partial[perm]):
        assert torch.equal(order.sum(0), torch.stack([b.dbeta, b.dgamma])), "fp32 sums of the backward partials are exact in any order"
    assert torch.equal(b.partial.double().sum(0), b.ints.sum(0).double())
    assert (b.dbeta != b.dgamma).all(), "swapped slots must be visible in every channel"
    assert int(b.ints.sum(0).abs().max()) < 2 ** 20


def test_finalize_cases_cover_the_regimes():
    """The tile counts sit on both sides of the one-launch | wide | two-stage boundaries and of the unrolled loops' tails."""
    t = set(X.FINALIZE_TILES)
    assert {1023, 1024, 1025, 16383, 16384, 16385} <= t and max(t) > 16384 + 64
    assert any(x <= 1024 and (x - 1) % 64 + 1 <= 48 for x in t) and any(x <= 1024 and x % 16 for x in t)      # one-launch kernel: tail trips
    wide = [x for x in t if 1024 < x <= 16384]
    assert any((x - 1) % 256 >= 192 for x in wide) and any((x - 1) % 256 < 192 for x in wide)
    assert {C for C, _ in X.FINALIZE_CASES} == {4, 64, 1024} and all(tl <= 1025 for C, tl in X.FINALIZE_CASES if C == 1024)


def _lane_loop(p, KL):
    """The lane regimes tile by tile, as the kernel text reads (p: [tiles][...] fp64)."""
    tiles, lanes = p.shape[0], []
    for k in range(KL):
        s, t = torch.zeros_like(p[0]), k
        while t + 3 * KL < tiles:
            s = s + ((p[t] + p[t + KL]) + (p[t + 2 * KL] + p[t + 3 * KL]))
            t += 4 * KL
        while t < tiles:
            s = s + p[t]
            t += KL
        lanes.append(s)
    tot = lanes[0]
    for k in range(1, KL):
        tot = tot + lanes[k]
    return tot


def _two_stage_loop(p):
    """Stage 1 + chunk sums tile by tile."""
    tiles = p.shape[0]
    S = min(max((tiles + 63) // 64, 1), 64)
    per = (tiles + S - 1) // S
    chunks = []
    for y in range(S):
        t0, t1 = y * per, min(tiles, (y + 1) * per)
        waves = []
        for w in range(4):
            s = torch.zeros_like(p[0])
            for t in range(t0 + w, t1, 4):
                s = s + p[t]
            waves.append(s)
        chunks.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    lanes = []
    for kl in range(4):
        s = torch.zeros_like(p[0])
        for j in range(16):
            s = s + (chunks[kl + 4 * j] if kl + 4 * j < S else 0.0)
        lanes.append(s)
    return ((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]


@pytest.mark.parametrize("tiles", [17, 1025 + 191])
def test_order_restatement_is_the_per_tile_loop(tiles):
    """exact.order_total (vectorised over lanes, one trip per step) against the direct per-tile loops above, for all three regimes."""
    c = X.reduce_case("cancelling", tiles, 4)
    for p in (c.fwd, c.bwd.double()):
        assert torch.equal(X.order_total(p, "narrow"), _lane_loop(p, 16))
        assert torch.equal(X.order_total(p, "wide"), _lane_loop(p, 64))
        assert torch.equal(X.order_total(p, "two_stage"), _two_stage_loop(p))


@pytest.mark.parametrize("C,tiles", [c for c in X.FINALIZE_CASES if c[1] > 64], ids=_ids)
def test_cancelling_partials_tell_orders_apart(C, tiles):
    """A condition on the inputs of test_finalize_order: on the cancelling partials the three regimes' orders and the plain sequential
    order give pairwise different totals in at least half of the channels of each slot, in both layouts -- so a kernel that adds in
    another regime's order, or tile by tile, cannot pass.  (At or below 64 tiles one or both lane regimes ARE the sequential order.)
    The totals are what the GPU test compares: float32(total) for the backward layout, float32(total / M) for the forward one."""
    c = X.reduce_case("cancelling", tiles, C)
    assert c.bwd.dtype == torch.float32 and c.fwd.dtype == torch.float64 and c.M == X.reduce_case("fwd_partials", tiles, C).M
    for name, p, scale in (("forward", c.fwd, 1.0 / c.M), ("backward", c.bwd, 1.0)):
        assert torch.isfinite(p).all()
        tot = {r: (X.order_total(p, r) * scale).float() for r in X.ORDER_REGIMES}
        tot["sequential"] = (X.sequential_total(p) * scale).float()
        assert tot[X.finalize_regime(tiles)].abs().max().item() < 1e-6 * p.abs().max().item() * scale, "the totals must be residue"
        names = list(tot)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                differ = (tot[a] != tot[b]).sum(1)
                assert (2 * differ >= C).all(), f"{name} {tiles} x {C}: {a} and {b} differ in {differ.tolist()} of {C} channels per slot"


@pytest.mark.parametrize("M,C", X.BN_ROW_CASES, ids=_ids)
def test_bn_rows(M, C):
    c = X.reduce_case("bn_rows", M, C)
    xd = c.x.double()
    s, q = X.bn_stat_sums(c)
    assert torch.equal(xd.sum(0), s.double()) and torch.equal((xd * xd).sum(0), q.double()), "forward statistics"
    xhat32 = (c.x - c.ch.mean) * c.ch.invstd
    xhat = (xd - c.ch.mean.double()) * c.ch.invstd.double()
    assert torch.equal(xhat32.double(), xhat) and torch.equal((c.g * xhat32).double(), c.g.double() * xhat), "xhat and g * xhat are exact in fp32"
    out = X.bn_apply_rows(c.x, c.ch, relu=True, residual=c.res)
    assert torch.equal(out.float().double(), out), "bn(x) + residual is exact in fp32"
    for mask in (None, out > 0):
        dg, db = X.bn_bwd_sums(c, mask)
        g = c.g if mask is None else c.g * mask
        assert torch.equal(g.double().sum(0), db.double()) and torch.equal((g.double() * xhat).sum(0), dg.double()), "backward sums, fp64"
        assert torch.equal(g.sum(0), db) and torch.equal((g * xhat32).sum(0), dg), "backward sums, fp32"
    if M >= 31:          # rows differ from one another in every channel (a handful of random rows may not)
        assert (c.gi != 0).any(0).all() and (c.dev.min(0).values != c.dev.max(0).values).all() and (c.gi.min(0).values != c.gi.max(0).values).all()


def test_bn_row_cases_cover_the_edges():
    ms = lambda C: set(X.bn_row_counts(C))
    for C in X.BN_C:
        nrl = 1024 // C
        assert {1, 31, 32, 33, 65} <= ms(C) and nrl + 1 in ms(C) and (nrl == 1 or nrl - 1 in ms(C))
    for C in (4, 64):
        wrap = X.BN_WRAP_N4 * 4 // C
        assert {65537, 2 ** 18 + 1, wrap} <= ms(C) and 8192 * 256 < wrap * C // 4 < 8192 * 256 + 4096, "the second grid-stride trip is a short tail"
    assert len(X.BN_ROW_CASES) == sum(len(ms(C)) for C in X.BN_C)


@pytest.mark.parametrize("geom,patch", X.DGRAD_BN_GEOMS, ids=_ids)
def test_dgrad_epilogue_inputs(geom, patch):
    c = X.reduce_case("dgrad_bn", geom)
    N, H, W, Cin, Cout, k, s, p = geom
    assert torch.equal(c.dx.double(), X.conv_dgrad(c.dy.double(), c.w.double(), (N, H, W, Cin), s, p)), "dx is exact in fp32"
    assert c.amax >= 1 and c.dx.abs().max().item() > 8
    for v in ((c.dx + c.res) * (c.msk > 0), c.dx * (c.msk > 0), c.dx):
        for q in range(2):
            dg, db = X.dgrad_bn_sums(c, v, q)
            xhat = (c.zs[q].double() - c.chs[q].mean.double()) * c.chs[q].invstd.double()
            assert torch.equal(v.double().reshape(-1, Cin).sum(0), db.double())
            assert torch.equal((v.double() * xhat).reshape(-1, Cin).sum(0), dg.double())
            assert torch.equal((v * xhat.float()).reshape(-1, Cin).sum(0), dg), "fp32 evaluation"
    assert not torch.equal(X.dgrad_bn_sums(c, c.dx, 0)[0], X.dgrad_bn_sums(c, c.dx, 1)[0]), "the two requests must differ"


@pytest.mark.parametrize("case", X.POOLED_CASES, ids=_ids)
def test_pooled_inputs(case):
    N, H, W, C = case
    c = X.reduce_case("pooled", *case)
    assert torch.equal(c.act.float().double(), c.act), "relu(bn(y)) is exact in fp32"
    idx = X.pooled_idx_cpu(c)
    dg, db, a_sel = X.pooled_sums(c, idx)
    pooled = torch.nn.functional.max_pool2d(c.act.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(a_sel, pooled), "the decoded decisions select the maxima"
    # the same sums in gather form: scatter the pooled gradient to the selected pixels, mask, reduce over PIXELS in fp64
    g = X.pooled_gather(c, idx).reshape(-1, C)
    xhat = ((c.y.double() - c.ch.mean.double()) * c.ch.invstd.double()).reshape(-1, C)
    assert torch.equal(g.sum(0), db.double()) and torch.equal((g * xhat).sum(0), dg.double())
    assert g.abs().max().item() <= 28
    assert 0.2 < (a_sel > 0).double().mean().item() < 1.0, "the ReLU mask must cut some of the selected pixels, not all"


@pytest.mark.parametrize("M,C", X.COLSUM_CASES, ids=_ids)
def test_colsum_inputs(M, C):
    c = X.reduce_case("colsum", M, C)
    assert torch.equal(c.x.double().sum(0), c.total.double()) and torch.equal(c.x.sum(0), c.total)
    assert torch.equal(c.x.flip(0).sum(0), c.total)


@pytest.mark.parametrize("M,D", X.LN_CASES, ids=_ids)
def test_layernorm_inputs(M, D):
    c = X.reduce_case("ln", M, D)
    xh32 = (c.x - c.mean[:, None]) * c.rstd[:, None]
    xh = (c.x.double() - c.mean.double()[:, None]) * c.rstd.double()[:, None]
    assert torch.equal(xh32.double(), xh) and torch.equal((c.dy * xh32).double(), c.dy.double() * xh), "xhat and dy * xhat are exact in fp32"
    assert torch.equal(c.dy.double().sum(0), c.db.double()) and torch.equal((c.dy.double() * xh).sum(0), c.dw.double())
    assert torch.equal(c.dy.sum(0), c.db) and torch.equal((c.dy * xh32).sum(0), c.dw), "fp32 evaluation"
    assert torch.equal((c.dy * c.w).double(), c.dy.double() * c.w.double())
    assert not torch.equal(c.db, c.dw)


def test_sum_budget_is_not_decoration():
    with pytest.raises(AssertionError, match="not exact"):
        X.assert_sum_budget(torch.tensor([5, 2 ** 24]))
    assert X.assert_sum_budget(torch.tensor([5, 2 ** 24 - 1])) < 24
    with pytest.raises(AssertionError, match="not representable"):
        X.exact_f32(torch.tensor([2 ** 24 + 1]), 1.0)
    r = X.rand_ints((1000,), -3, 3, 1, nonzero=True)
    assert (r != 0).all() and int(r.min()) == -3 and int(r.max()) == 3
