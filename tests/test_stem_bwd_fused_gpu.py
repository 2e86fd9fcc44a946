"""The stem weight gradient that forms conv1's gradient itself (mla_conv2d_stem_wgrad_split_bnpool): the apply pass of the stem's
BatchNorm / max-pool backward runs where the plain kernel loads dy.

  1. bit for bit the un-fused sequence mla_bn_bwd_pooled -> mla_conv2d_stem_wgrad_split (dw, dgamma, dbeta);
  2. the CPU oracle's conv1 weight gradient through bn1 / relu / maxpool, at the tolerance of test_stem_split_fwd_wgrad (2e-5 of
     max|ref|: the conv contraction's; the BatchNorm backward's own rounding, ~1e-6 of max|dy| per element, averages out below it);
  3. a whole encoder backward with the path on and off: every gradient bitwise equal, no DY["conv1"] buffer when on;
  4. argument checks.

Shapes: the smallest that reach every branch -- odd OH, partial 16 x 16 tiles in both directions, a last pooled window that is
partly outside, both Cin, and one case with more tiles than CUs (a workgroup walks >= 2 tiles: the dy stream crosses a tile boundary).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from util import assert_close  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _cus(ops):
    """The CU count the persistent stem grids use: the weight-gradient workspace is one [49 Cin][64] fp32 slab per CU."""
    return ops.conv2d_stem_wgrad_split_ws_bytes(1) // (49 * 64 * 4)


def _stem_case(ops, N, H, W, Cin, seed):
    """Inputs as the step forms them: y from the forward kernel, statistics from the real finalize, codes from the real max-pool."""
    x = O.portable_normal(seed, (N, Cin, H, W), stream=1)
    w = O.portable_normal(seed, (64, Cin, 7, 7), stream=2, std=math.sqrt(2.0 / (Cin * 49)))
    gamma = O.portable_normal(seed, (64,), stream=3, mean=0.3, std=1.0)          # mixed sign
    beta = O.portable_normal(seed, (64,), stream=4, std=0.3)
    gamma[5] = 0.0                                                                # bn(y) = beta: the ReLU mask is decided by beta alone
    assert (gamma > 0).any() and (gamma < 0).any()
    xd, wd = nhwc(x).cuda(), w.permute(2, 3, 1, 0).contiguous().cuda()
    part = torch.zeros(ops.conv2d_stem_fwd_partial_elems(), device="cuda")
    y, tiles = ops.conv2d_stem_fwd_split(xd, wd, bn_partial=part)
    M = y.numel() // 64
    mean, invstd = torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    ops.bn_finalize(part, tiles, M, 64, mean, invstd, None, None)
    ga, be = gamma.cuda(), beta.cuda()
    OH, OW = y.shape[1], y.shape[2]
    PH, PW = ops.conv_out(OH, 3, 2, 1), ops.conv_out(OW, 3, 2, 1)
    p = torch.empty((N, PH, PW, 64), device="cuda")
    idx = torch.empty((N, PH, PW, 64), device="cuda", dtype=torch.uint8)
    ops.bn_relu_maxpool_fwd(y, mean, invstd, ga, be, p, idx)
    dpool = O.portable_normal(seed, (N, 64, PH, PW), stream=5)
    dpool[O.portable_normal(seed, (N, 64, PH, PW), stream=6).abs() < 0.1257] = 0.0     # about a tenth exactly zero
    return dict(x=x, xd=xd, y=y, mean=mean, invstd=invstd, gamma=gamma, beta=beta, ga=ga, be=be, idx=idx, dpool=dpool,
                dpd=nhwc(dpool).cuda(), Cin=Cin, M=M)


def _unfused(ops, c):
    dy, dg, db = torch.empty_like(c["y"]), torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    ws_bn = torch.empty(ops.bn_bwd_ws_elems(c["M"], 64), device="cuda")
    ops.bn_bwd_pooled(c["dpd"], c["idx"], c["y"], c["mean"], c["invstd"], c["ga"], c["be"], dy, dg, db, ws_bn)
    dw = torch.empty((7, 7, c["Cin"], 64), device="cuda")
    ws = torch.empty(ops.conv2d_stem_wgrad_split_ws_bytes(c["Cin"]) // 4, device="cuda")
    ops.conv2d_stem_wgrad_split(c["xd"], dy, dw, 2, 3, ws)
    return dw, dg, db


def _fused(ops, c):
    dg, db = torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    ws_bn = torch.empty(ops.bn_bwd_ws_elems(c["M"], 64), device="cuda")
    ops.bn_bwd_pooled(c["dpd"], c["idx"], c["y"], c["mean"], c["invstd"], c["ga"], c["be"], None, dg, db, ws_bn)
    dw = torch.full((7, 7, c["Cin"], 64), float("nan"), device="cuda")
    ws = torch.empty(ops.conv2d_stem_wgrad_split_ws_bytes(c["Cin"]) // 4, device="cuda")
    ops.conv2d_stem_wgrad_split_bnpool(c["xd"], c["dpd"], c["idx"], c["y"], c["mean"], c["invstd"], c["ga"], c["be"], dg, db, dw, ws)
    return dw, dg, db


def _oracle_dw(ops, c):
    """conv1's weight gradient through bn1 / relu / maxpool on the CPU, from the forward output the kernels saw and with the HIP
    path's own max-pool and ReLU decisions (flip-immune, as test_stem_fused)."""
    y = nchw(c["y"].cpu())
    N, _, OH, OW = y.shape
    a = torch.empty_like(c["y"])
    ops.bn_apply(c["y"].view(c["M"], 64), c["mean"], c["invstd"], c["ga"], c["be"], a.view(c["M"], 64), c["M"], 64, True)
    code = nchw(c["idx"].cpu()).long()
    PH, PW = code.shape[2], code.shape[3]
    oy = torch.arange(PH).view(1, 1, PH, 1)
    ox = torch.arange(PW).view(1, 1, 1, PW)
    flat = (oy * 2 - 1 + code // 3) * OW + (ox * 2 - 1 + code % 3)
    g = O.maxpool3x3s2_bwd(c["dpool"], flat, y.shape) * (nchw(a.cpu()) > 0)
    _, mean_ref, invstd_ref = O.bn_train_fwd(y, c["gamma"], c["beta"], torch.zeros(64), torch.ones(64))
    dy_ref, _, _ = O.bn_train_bwd(g, y, c["gamma"], mean_ref, invstd_ref)
    return O.conv2d_wgrad(c["x"], dy_ref.float(), (64, c["Cin"], 7, 7), 2, 3)


def _cases():
    return [pytest.param(2, 70, 38, 1, id="audio-35x19"),           # odd OH, partial tiles both ways, last pooled window partly outside
            pytest.param(3, 46, 62, 3, id="visual-23x31"),
            pytest.param(2, 64, 32, 1, id="audio-whole-tiles"),    # multiples of 16: the kernels without per-pixel range checks
            pytest.param(1, 32, 64, 3, id="visual-whole-tiles"),
            pytest.param(0, 130, 130, 3, id="visual-multi-tile")]   # N chosen below: more tiles than CUs


@pytest.mark.parametrize("N,H,W,Cin", _cases())
def test_fused_equals_unfused_and_oracle(ops, N, H, W, Cin):
    if N == 0:
        per = ((65 + 15) // 16) ** 2                                    # 25 tiles per image
        N = max(4, _cus(ops) // per + 1)
        assert N * per > _cus(ops)
    c = _stem_case(ops, N, H, W, Cin, seed=N + H + W + Cin)
    dw_u, dg_u, db_u = _unfused(ops, c)
    dw_f, dg_f, db_f = _fused(ops, c)
    torch.cuda.synchronize()
    assert torch.equal(dg_f, dg_u) and torch.equal(db_f, db_u), "the reduction half alone must give the same dgamma / dbeta"
    d = (dw_f - dw_u).abs().max().item()
    print(f"fused vs unfused max|d| = {d:.3e}")
    assert torch.equal(dw_f, dw_u), f"fused stem weight gradient differs from bn_bwd_pooled -> stem_wgrad_split (max|d| = {d:.3e})"
    dw_ref = _oracle_dw(ops, c)
    err = assert_close(dw_f.permute(3, 2, 0, 1).cpu(), dw_ref, atol=0, rtol=2e-5, name="fused stem wgrad vs oracle")
    print(f"fused vs oracle max|d| = {err:.3e} (max|ref| = {dw_ref.abs().max().item():.3e})")
    dw_2, _, _ = _fused(ops, c)
    assert torch.equal(dw_f, dw_2), "bitwise reproducible"


@pytest.mark.parametrize("side", [False, True], ids=["one-stream", "side-stream"])
def test_encoder_backward_fused_equals_unfused(side):
    """One small encoder forward + backward with MLA_STEM_BWD_FUSE on and off (the instance switch the variable sets): every
    gradient bit for bit, and the fused run holds no DY["conv1"]."""
    from mla_hip.encoder import ResNet18Encoder
    x = O.portable_normal(1, (2, 1, 64, 32), stream=1).cuda()
    dfeat = O.portable_normal(1, (2, 512), stream=3).cuda()
    grads = {}
    for fuse in (True, False):
        enc = ResNet18Encoder("audio", "cuda", seed=7, conv_math="split")
        assert enc.stem_bwd_fuse, "the fused stem backward is the default on the split arithmetic"
        enc.stem_bwd_fuse = fuse
        if side:
            enc.wgrad_stream = torch.cuda.Stream()
        enc.train()
        feat = enc.forward(x)
        enc.backward_from_pooled(dfeat, feat.shape[1] * feat.shape[2])
        torch.cuda.synchronize()
        assert ("conv1" in enc._ws["DY"]) == (not fuse)
        grads[fuse] = {k: v.clone() for k, v in enc.g.items()}
    for k in grads[True]:
        assert torch.equal(grads[True][k], grads[False][k]), k
    for math_ in ("f32", "bf16"):
        assert not ResNet18Encoder("audio", "cuda", seed=7, conv_math=math_).stem_bwd_fuse, "f32 / bf16 keep the two-kernel path"


def test_argument_checks(ops):
    """Null pointers, a workspace that is too small and Cout != 64 come back as error codes (nothing is launched: dw stays as it was)."""
    from mla_hip import _lib
    lib = _lib.load()
    c = _stem_case(ops, 1, 32, 32, 1, seed=3)
    dg, db = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    dw = torch.full((7, 7, 1, 64), 7.0, device="cuda")
    ws = torch.empty(ops.conv2d_stem_wgrad_split_ws_bytes(1) // 4, device="cuda")
    ptrs = [c["xd"], c["dpd"], c["idx"], c["y"], c["mean"], c["invstd"], c["ga"], c["be"], dg, db, dw]

    def call(p, cout=64, ws_bytes=ws.numel() * 4, ws_ptr=ws.data_ptr()):
        return lib.mla_conv2d_stem_wgrad_split_bnpool(*p, 1, 32, 32, 1, cout, 7, 7, 2, 3, ws_ptr, ws_bytes, None)
    good = [t.data_ptr() for t in ptrs]
    for k in range(len(good)):
        assert call(good[:k] + [None] + good[k + 1:]) == -1, f"null pointer in position {k}"
        assert b"null pointer" in lib.mla_last_error()
    assert call(good, ws_ptr=None) == -1
    assert call(good, cout=128) == -1
    assert call(good, ws_bytes=49 * 64 * 4 - 4) == -2                  # one slab (the single tile's) needs 49 * 64 floats
    assert b"workspace" in lib.mla_last_error()
    torch.cuda.synchronize()
    assert (dw == 7.0).all(), "a refused call must not launch"
    assert call(good) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dw).all() and not (dw == 7.0).all()
