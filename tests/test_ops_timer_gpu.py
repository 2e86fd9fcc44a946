"""The records ops.KernelTimer collects for bench.py's roofline: one (kind, work, moved) per timed wrapper call.

The expected numbers are written out from the formulas of the wrappers (work = 2 * output elements * KH * KW * Cin for the
contractions, bytes per element for the BatchNorm passes), not obtained from ops.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# 64-channel convolutions: N=2, H=W=8, Cin=Cout=64, 3x3 / 1 / 1 -> 2 * (2*8*8*64) * 9 * 64; BatchNorm on the same tensor: M=128, C=64
CONV = 9437184.0
# BatchNorm passes on M * C = 128 * 64 = 8192 elements: 8 / 12 / 20 bytes per element -> 65536 / 98304 / 163840; the pooled stem passes
# add 5 / 10 bytes per pooled element (2 * 4 * 4 * 64 = 2048): 4 * 8192 + 5 * 2048 = 43008, 12 * 8192 + 10 * 2048 = 118784
# folded-BatchNorm kernels at test_ops_gpu.py's smallest fold case (3, 20, 12): 2 * (3*20*12*64) * 9 * 64
FOLD = 53084160.0
# stem at test_ops_gpu.py's smallest stem case (1, 7, 9, 3): 4 x 5 outputs -> 2 * (1*4*5*64) * 49 * 3
STEM = 376320.0

EXPECTED = [
    ("conv_fwd", CONV, 0.0),                    # conv2d_fwd
    ("bn_fwd", 0.0, 0.0),                       # bn_finalize
    ("bn_fwd", 98304.0, 65536.0),               # bn_apply
    ("bn_fwd", 98304.0, 98304.0),               # bn_apply with a residual
    ("conv_fwd", CONV, 0.0),                    # conv2d_fwd_split
    ("conv_dgrad", CONV, 0.0),                  # conv2d_dgrad
    ("conv_dgrad", CONV, 0.0),                  # conv2d_dgrad_split (with a BatchNorm reduction request)
    ("bn_bwd", 98304.0, 98304.0),               # bn_bwd_from_partial
    ("bn_bwd", 163840.0, 163840.0),             # bn_bwd
    ("conv_wgrad", CONV, 0.0),                  # conv2d_wgrad
    ("conv_wgrad", CONV, 0.0),                  # conv2d_wgrad_split
    ("bn_fwd", 43008.0, 43008.0),               # bn_relu_maxpool_fwd: (2, 8, 8, 64) -> (2, 4, 4, 64)
    ("bn_bwd", 118784.0, 118784.0),             # bn_bwd_pooled
    ("conv_fwd", FOLD, 0.0),                    # conv2d_fwd_split_bnin
    ("conv_wgrad", FOLD, 0.0),                  # conv2d_wgrad_split_bnin
    ("conv_dgrad", FOLD, 0.0),                  # conv2d_dgrad_split_bnmask
    ("stem_fwd", STEM, 0.0),                    # conv2d_stem_fwd_split
    ("stem_wgrad", STEM, 0.0),                  # conv2d_stem_wgrad_split
]


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _every_timed_wrapper(ops):
    """Each timed wrapper once, in the order of EXPECTED, on fixed inputs and fresh outputs; returns what the wrappers returned."""
    g = torch.Generator(device="cuda").manual_seed(11)

    def rnd(*shape):
        return torch.randn(shape, device="cuda", generator=g)

    def f32(*shape):
        return torch.empty(shape, device="cuda")

    ret = []
    N, H, W, C, M = 2, 8, 8, 64, 128
    x, dy, res, w = rnd(N, H, W, C), rnd(N, H, W, C), rnd(M, C), rnd(3, 3, C, C) * 0.06
    gamma, beta = rnd(C) * 0.2 + 1.0, rnd(C) * 0.3
    wT, wS = ops.conv2d_wsplit(w, True), ops.conv2d_wsplit(w, False)
    part = torch.zeros(ops.conv2d_fwd_partial_elems(N, H, W, C, C, 3, 3, 1, 1), device="cuda")
    y, tiles = ops.conv2d_fwd(x, w, 1, 1, bn_partial=part)
    ret.append((y, tiles))
    mean, invstd = f32(C), f32(C)
    ret.append(ops.bn_finalize(part, tiles, M, C, mean, invstd, None, None))
    ret += [mean, invstd]
    a = ops.bn_apply(y.view(M, C), mean, invstd, gamma, beta, f32(M, C), M, C, True)
    ret.append(a)
    ret.append(ops.bn_apply(y.view(M, C), mean, invstd, gamma, beta, f32(M, C), M, C, False, residual=res))
    ret.append(ops.conv2d_fwd_split(x, wT, w.shape, 1, 1))
    ret.append(ops.conv2d_dgrad(dy, w, (N, H, W, C), 1, 1, f32(w.numel()), relu_src=a.view(N, H, W, C)))
    bnp = torch.zeros(ops.conv2d_dgrad_bn_partial_elems(N, H, W, C), device="cuda")
    dx, rt = ops.conv2d_dgrad_split(dy, wS, w.shape, (N, H, W, C), 1, 1, bn_reqs=[(y, mean, invstd, bnp)])
    ret.append((dx, rt))
    d1, dg, db = f32(M, C), f32(C), f32(C)
    ret.append(ops.bn_bwd_from_partial(dx.view(M, C), y.view(M, C), mean, invstd, gamma, d1, dg, db, bnp, rt, M, C))
    ret += [d1, dg.clone(), db.clone()]
    bn_ws = f32(ops.bn_bwd_ws_elems(M, C))
    d2 = f32(M, C)
    ret.append(ops.bn_bwd(dy.view(M, C), y.view(M, C), mean, invstd, gamma, d2, dg, db, bn_ws, M, C))
    ret += [d2, dg.clone(), db.clone()]
    ws = f32(max(ops.conv2d_wgrad_ws_bytes(N, H, W, C, C, 3, 3, 1, 1), ops.conv2d_wgrad_split_ws_bytes(N, H, W, C, C, 3, 3, 1, 1)) // 4 + 4)
    ret.append(ops.conv2d_wgrad(x, dy, f32(3, 3, C, C), 1, 1, ws))
    ret.append(ops.conv2d_wgrad_split(x, dy, f32(3, 3, C, C), 1, 1, ws))
    pool, idx = f32(N, 4, 4, C), torch.empty((N, 4, 4, C), device="cuda", dtype=torch.uint8)
    ret.append(ops.bn_relu_maxpool_fwd(y, mean, invstd, gamma, beta, pool, idx))
    ret += [pool, idx]
    d3 = f32(N, H, W, C)
    ret.append(ops.bn_bwd_pooled(rnd(N, 4, 4, C), idx, y, mean, invstd, gamma, beta, d3, dg, db, bn_ws))
    ret += [d3, dg.clone(), db.clone()]

    # folded BatchNorm: relu(bn(y1)) re-formed inside the 64 -> 64 kernels (the patch kernel wherever the geometry allows)
    N, H, W = 3, 20, 12
    y1, dy1 = rnd(N, H, W, C) * 1.3 + 0.2, rnd(N, H, W, C)
    m1 = y1.mean((0, 1, 2)).contiguous()
    i1 = torch.rsqrt(y1.var((0, 1, 2), unbiased=False) + ops.BN_EPS).contiguous()
    default_patch = ops.conv2d_patch()
    ops.conv2d_patch(2)
    try:
        ret.append(ops.conv2d_fwd_split_bnin(y1, wT, w.shape, 1, 1, (m1, i1, gamma, beta)))
        ws = f32(ops.conv2d_wgrad_split_ws_bytes(N, H, W, C, C, 3, 3, 1, 1) // 4 + 4)
        ret.append(ops.conv2d_wgrad_split_bnin(y1, dy1, f32(3, 3, C, C), 1, 1, ws, (m1, i1, gamma, beta)))
        bnp = torch.zeros(ops.conv2d_dgrad_bn_partial_elems(N, H, W, C), device="cuda")
        ret.append(ops.conv2d_dgrad_split_bnmask(dy1, wS, w.shape, (N, H, W, C), 1, 1, f32(N, H, W, C), (y1, m1, i1, bnp), gamma, beta))
    finally:
        ops.conv2d_patch(default_patch)

    # stem
    xs, w7 = rnd(1, 7, 9, 3), rnd(7, 7, 3, 64) * 0.1
    ys, ts = ops.conv2d_stem_fwd_split(xs, w7, bn_partial=torch.zeros(ops.conv2d_stem_fwd_partial_elems(), device="cuda"))
    ret.append((ys, ts))
    ws = f32(ops.conv2d_stem_wgrad_split_ws_bytes(3) // 4)
    ret.append(ops.conv2d_stem_wgrad_split(xs, rnd(*ys.shape), f32(7, 7, 3, 64), 2, 3, ws))
    torch.cuda.synchronize()
    return ret


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    return type(a) is type(b) and a == b


def test_timer_records_and_timer_off(ops, monkeypatch):
    made = []
    real_event = torch.cuda.Event

    def counting_event(*args, **kwargs):
        made.append(1)
        return real_event(*args, **kwargs)

    monkeypatch.setattr(torch.cuda, "Event", counting_event)
    assert ops.TIMER is None
    off = _every_timed_wrapper(ops)
    assert not made, "with the timer off no event is created"
    timer = ops.KernelTimer()
    ops.TIMER = timer
    try:
        on = _every_timed_wrapper(ops)
    finally:
        ops.TIMER = None
    records = [(kind, work, moved) for kind, work, _s, _e, moved in timer.records]
    for k, (got, want) in enumerate(zip(records, EXPECTED)):
        print(k, got, want)
    assert records == EXPECTED
    assert len(made) == 2 * len(EXPECTED), "one begin and one end event per record"
    assert all(s.elapsed_time(e) >= 0.0 for _k, _w, s, e, _m in timer.records), "begin is recorded before end, on the launch's stream"
    assert len(off) == len(on) and all(_same(a, b) for a, b in zip(off, on)), "the timer must not change what the wrappers return"
    # the per-kind sums bench.py's roofline reads
    summary = timer.summary()
    for kind in {k for k, _w, _m in EXPECTED}:
        rows = [(w, m) for k, w, m in EXPECTED if k == kind]
        assert summary[kind]["launches"] == len(rows)
        assert summary[kind]["work"] == sum(w for w, _m in rows) and summary[kind]["moved"] == sum(m for _w, m in rows)
    made.clear()
    _every_timed_wrapper(ops)
    assert not made and len(timer.records) == len(EXPECTED), "timer off again: no events, and the old timer receives nothing"
