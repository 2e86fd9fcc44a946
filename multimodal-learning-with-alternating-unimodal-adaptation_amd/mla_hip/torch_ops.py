"""`torch.ops.mla_hip.*`: the C-ABI launchers registered as PyTorch custom ops.

`torch.library` registrations (dispatch key CUDA = HIP on ROCm) over the ctypes launchers in ops.py: each op allocates
its outputs with torch, enqueues the kernel(s) on the current stream and returns -- no synchronisation, no fallback
implementation for any other dispatch key (calling one with CPU tensors raises torch's "no kernel" error, loudly).
Functional ops return new tensors; ops that update state take it as a mutable argument (`Tensor(a!)`), exactly what the
launcher does.  Layouts are the kernels': activations NHWC, conv weights HWIO, Linear weights [in][out].

The nn.Module / autograd.Function boundary (model.py, autograd.py) drives the same launchers through launch plans with
preallocated workspaces; these ops are the operator-level surface for code that composes the kernels itself.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import ops

_lib = torch.library.Library("mla_hip", "DEF")
_defined: List[str] = []


def _op(schema: str):
    name = schema.split("(", 1)[0]
    _lib.define(schema)

    def deco(fn):
        _lib.impl(name, fn, "CUDA")
        _defined.append(name)
        return fn
    return deco


def op_names() -> List[str]:
    return list(_defined)


def _f32(shape, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(shape, device=like.device, dtype=torch.float32)


# ---- convolution (nn.Conv2d, backbone.py:4-12) -------------------------------------------------------------------
@_op("conv2d_fwd(Tensor x, Tensor w_hwio, int stride, int pad, str math='f32') -> Tensor")
def conv2d_fwd(x, w_hwio, stride, pad, math="f32"):
    if math == "split":
        return ops.conv2d_fwd_split(x, ops.conv2d_wsplit(w_hwio, True), tuple(w_hwio.shape), stride, pad)[0]
    return ops.conv2d_fwd(x, w_hwio, stride, pad)[0]


@_op("conv2d_fwd_stats(Tensor x, Tensor w_hwio, int stride, int pad) -> (Tensor, Tensor, Tensor)")
def conv2d_fwd_stats(x, w_hwio, stride, pad):
    """conv + the BatchNorm batch statistics of its output from the conv epilogue: (y, mean, invstd)."""
    N, H, W, Cin = x.shape
    KH, KW, _, Cout = w_hwio.shape
    part = _f32(ops.conv2d_fwd_partial_elems(N, H, W, Cin, Cout, KH, KW, stride, pad), x)
    y, tiles = ops.conv2d_fwd(x, w_hwio, stride, pad, bn_partial=part)
    M = y.numel() // Cout
    mean, invstd = _f32(Cout, x), _f32(Cout, x)
    ops.bn_finalize(part, tiles, M, Cout, mean, invstd, None, None)
    return y, mean, invstd


@_op("conv2d_dgrad(Tensor dy, Tensor w_hwio, int[] x_shape, int stride, int pad, Tensor? residual=None, Tensor? relu_src=None) -> Tensor")
def conv2d_dgrad(dy, w_hwio, x_shape, stride, pad, residual=None, relu_src=None):
    return ops.conv2d_dgrad(dy, w_hwio, tuple(x_shape), stride, pad, _f32(w_hwio.numel(), dy), residual=residual,
                            relu_src=relu_src)


@_op("conv2d_wgrad(Tensor x, Tensor dy, int[] w_shape, int stride, int pad) -> Tensor")
def conv2d_wgrad(x, dy, w_shape, stride, pad):
    N, H, W, Cin = x.shape
    KH, KW, _, Cout = w_shape
    ws = _f32(ops.conv2d_wgrad_ws_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad) // 4 + 4, x)
    return ops.conv2d_wgrad(x, dy, _f32(tuple(w_shape), x), stride, pad, ws)


# ---- the same convolutions on the single-product bf16 arithmetic (conv_math "bf16") -------------------------------------------
@_op("conv2d_fwd_bf16(Tensor x, Tensor w_hwio, int stride, int pad) -> Tensor")
def conv2d_fwd_bf16(x, w_hwio, stride, pad):
    return ops.conv2d_fwd_bf16(x, ops.conv2d_wimage_bf16(w_hwio, True), tuple(w_hwio.shape), stride, pad)[0]


@_op("conv2d_dgrad_bf16(Tensor dy, Tensor w_hwio, int[] x_shape, int stride, int pad, Tensor? residual=None, Tensor? relu_src=None) -> Tensor")
def conv2d_dgrad_bf16(dy, w_hwio, x_shape, stride, pad, residual=None, relu_src=None):
    return ops.conv2d_dgrad_bf16(dy, ops.conv2d_wimage_bf16(w_hwio, False), tuple(w_hwio.shape), tuple(x_shape), stride, pad,
                                 residual=residual, relu_src=relu_src)


@_op("conv2d_wgrad_bf16(Tensor x, Tensor dy, int[] w_shape, int stride, int pad) -> Tensor")
def conv2d_wgrad_bf16(x, dy, w_shape, stride, pad):
    N, H, W, Cin = x.shape
    KH, KW, _, Cout = w_shape
    ws = _f32(ops.conv2d_wgrad_ws_bytes_bf16(N, H, W, Cin, Cout, KH, KW, stride, pad) // 4 + 4, x)
    return ops.conv2d_wgrad_bf16(x, dy, _f32(tuple(w_shape), x), stride, pad, ws)


# ---- batch norm (+ ReLU + residual add), training mode (backbone.py:29-50) ------------------------------------------
@_op("bn_act_fwd(Tensor y, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta, bool relu, Tensor? residual=None) -> Tensor")
def bn_act_fwd(y, mean, invstd, gamma, beta, relu, residual=None):
    C = y.shape[-1]
    return ops.bn_apply(y, mean, invstd, gamma, beta, torch.empty_like(y), y.numel() // C, C, relu, residual=residual)


@_op("bn_act_bwd(Tensor dout, Tensor y, Tensor mean, Tensor invstd, Tensor gamma) -> (Tensor, Tensor, Tensor)")
def bn_act_bwd(dout, y, mean, invstd, gamma):
    """(dy, dgamma, dbeta); `dout` must already carry the ReLU mask of the layer's output (the producing kernels fuse it)."""
    C = y.shape[-1]
    M = y.numel() // C
    dx, dg, db = torch.empty_like(y), _f32(C, y), _f32(C, y)
    ops.bn_bwd(dout, y, mean, invstd, gamma, dx, dg, db, _f32(ops.bn_bwd_ws_elems(M, C), y), M, C)
    return dx, dg, db


# ---- pooling (backbone.py:88, 152; basic_model.py:56-65) ----------------------------------------------------------------
@_op("maxpool3x3s2_fwd(Tensor x) -> (Tensor, Tensor)")
def maxpool3x3s2_fwd(x):
    N, H, W, C = x.shape
    oh, ow = ops.conv_out(H, 3, 2, 1), ops.conv_out(W, 3, 2, 1)
    y = _f32((N, oh, ow, C), x)
    idx = torch.empty((N, oh, ow, C), device=x.device, dtype=torch.uint8)
    ops.maxpool_fwd(x, y, idx)
    return y, idx


@_op("maxpool3x3s2_bwd(Tensor dy, Tensor idx, int[] x_shape, Tensor? relu_src=None) -> Tensor")
def maxpool3x3s2_bwd(dy, idx, x_shape, relu_src=None):
    dx = _f32(tuple(x_shape), dy)
    ops.maxpool_bwd(dy, idx, dx, tuple(x_shape), relu_src=relu_src)
    return dx


@_op("conv2d_dgrad_bn(Tensor dy, Tensor w_hwio, int[] x_shape, int stride, int pad, Tensor bn_x, Tensor bn_mean, Tensor bn_invstd, "
     "Tensor? residual=None, Tensor? relu_src=None) -> (Tensor, Tensor, int)")
def conv2d_dgrad_bn(dy, w_hwio, x_shape, stride, pad, bn_x, bn_mean, bn_invstd, residual=None, relu_src=None):
    """Input gradient whose epilogue also forms the reduction pass of the BatchNorm backward that consumes dx
    (bn_x = that BatchNorm's input): returns (dx, partial sums, tiles) for bn_bwd_from_partial."""
    N, H, W, Cin = x_shape
    wt_ws = _f32((w_hwio.numel(),), dy)
    part = _f32((ops.conv2d_dgrad_bn_partial_elems(N, H, W, Cin),), dy)
    dx, tiles = ops.conv2d_dgrad(dy, w_hwio, tuple(x_shape), stride, pad, wt_ws, residual=residual, relu_src=relu_src,
                                 bn_reqs=[(bn_x, bn_mean, bn_invstd, part)])
    return dx, part, tiles


@_op("bn_bwd_from_partial(Tensor dout, Tensor x, Tensor mean, Tensor invstd, Tensor gamma, Tensor partial, int tiles) -> (Tensor, Tensor, Tensor)")
def bn_bwd_from_partial(dout, x, mean, invstd, gamma, partial, tiles):
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x)
    dg, db = _f32((C,), x), _f32((C,), x)
    ops.bn_bwd_from_partial(dout, x, mean, invstd, gamma, dx, dg, db, partial, tiles, M, C)
    return dx, dg, db


@_op("bn_relu_maxpool_fwd(Tensor y, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta) -> (Tensor, Tensor)")
def bn_relu_maxpool_fwd(y, mean, invstd, gamma, beta):
    """maxpool3x3s2(relu(bn(y))) for the stem (backbone.py:150-152) without materialising the ReLU output."""
    N, H, W, C = y.shape
    oh, ow = ops.conv_out(H, 3, 2, 1), ops.conv_out(W, 3, 2, 1)
    out = _f32((N, oh, ow, C), y)
    idx = torch.empty((N, oh, ow, C), device=y.device, dtype=torch.uint8)
    ops.bn_relu_maxpool_fwd(y, mean, invstd, gamma, beta, out, idx)
    return out, idx


@_op("bn_bwd_pooled(Tensor dpool, Tensor idx, Tensor y, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta) -> (Tensor, Tensor, Tensor)")
def bn_bwd_pooled(dpool, idx, y, mean, invstd, gamma, beta):
    """Backward of bn_relu_maxpool_fwd: (dy, dgamma, dbeta)."""
    N, H, W, C = y.shape
    dy = torch.empty_like(y)
    dg, db = _f32((C,), y), _f32((C,), y)
    ws = _f32((ops.bn_bwd_ws_elems(N * H * W, C),), y)
    ops.bn_bwd_pooled(dpool, idx, y, mean, invstd, gamma, beta, dy, dg, db, ws)
    return dy, dg, db


@_op("avgpool_fwd(Tensor x, int groups) -> Tensor")
def avgpool_fwd(x, groups):
    """x (..., C) viewed as (groups, P, C) -> (groups, C): adaptive_avg_pool2d / 3d + flatten."""
    C = x.shape[-1]
    P = x.numel() // (groups * C)
    y = _f32((groups, C), x)
    ops.avgpool_fwd(x, y, groups, P, C)
    return y


@_op("avgpool_bwd(Tensor dy, int[] x_shape, Tensor? relu_src=None) -> Tensor")
def avgpool_bwd(dy, x_shape, relu_src=None):
    NB, C = dy.shape
    dx = _f32(tuple(x_shape), dy)
    ops.avgpool_bwd(dy, dx, NB, dx.numel() // (NB * C), C, relu_src=relu_src)
    return dx


# ---- shared head, cross entropy, projection, optimiser (main.py:432-440; utils/utils.py:24-41) ----------------------------
@_op("head_ce_fwd_bwd(Tensor X, Tensor W, Tensor b, Tensor labels, float inv_batch) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
def head_ce_fwd_bwd(X, W, b, labels, inv_batch):
    """(logits, loss[1], dW, db, dX)"""
    B, D = X.shape
    C = W.shape[0]
    logits, loss, dW, db, dX = _f32((B, C), X), _f32(1, X), _f32((C, D), X), _f32(C, X), _f32((B, D), X)
    ops.head_ce_fwd_bwd(X, W, b, labels, logits, loss, dW, db, dX, _f32(ops.head_ws_elems(B, C), X), inv_batch)
    return logits, loss, dW, db, dX


@_op("concat_head_ce_fwd_bwd(Tensor[] xs, Tensor W, Tensor b, Tensor labels, float inv_batch) -> "
     "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor[])")
def concat_head_ce_fwd_bwd(xs, W, b, labels, inv_batch):
    """Joint head (main.py:273-311): (out, out_m (M, B, C), loss[1], loss_m[M], dW, db, [dX_m])"""
    M, (B, D), C = len(xs), xs[0].shape, W.shape[0]
    x0 = xs[0]
    out, out_m, loss, loss_m = _f32((B, C), x0), _f32((M, B, C), x0), _f32(1, x0), _f32(M, x0)
    dW, db, dxs = _f32((C, M * D), x0), _f32(C, x0), [_f32((B, D), x0) for _ in range(M)]
    ops.concat_head_ce_fwd_bwd(list(xs), W, b, labels, out, out_m, loss, loss_m, dW, db, dxs,
                               _f32(ops.concat_head_ws_elems(B, C, M), x0), inv_batch)
    return out, out_m, loss, loss_m, dW, db, dxs


@_op("concat_head_fwd(Tensor[] xs, Tensor W, Tensor b) -> (Tensor, Tensor)")
def concat_head_fwd(xs, W, b):
    """(out, out_m (M, B, C)) = fc_out(cat(xs)) and the per-modality block products + b / M"""
    M, (B, _D), C = len(xs), xs[0].shape, W.shape[0]
    out, out_m = _f32((B, C), xs[0]), _f32((M, B, C), xs[0])
    ops.concat_head_fwd(list(xs), W, b, out, out_m)
    return out, out_m


@_op("concat_head_bwd(Tensor[] xs, Tensor W, Tensor dlogits, float scale=1.0) -> (Tensor, Tensor, Tensor[])")
def concat_head_bwd(xs, W, dlogits, scale=1.0):
    """(dW, db, [dX_m]) of the concatenated fc_out for a given d out, times `scale`"""
    M, (B, D), C = len(xs), xs[0].shape, W.shape[0]
    dW, db, dxs = _f32((C, M * D), xs[0]), _f32(C, xs[0]), [_f32((B, D), xs[0]) for _ in range(M)]
    ops.concat_head_bwd(list(xs), W, dlogits, dW, db, dxs, scale)
    return dW, db, dxs


# ---- sum / FiLM / gated fusion heads (fusion_modules.py:5-13, 38-67, 70-98) -------------------------------------------------------
def _fusion_ws(x, C):
    return _f32(ops.fusion_ws_elems(x.shape[0], x.shape[1], C), x)


@_op("fusion_sum_ce_fwd_bwd(Tensor x, Tensor y, Tensor Wx, Tensor bx, Tensor Wy, Tensor by, Tensor labels, float inv_batch, "
     "float bias_scale=1.0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def fusion_sum_ce_fwd_bwd(x, y, Wx, bx, Wy, by, labels, inv_batch, bias_scale=1.0):
    """(out, out_a, out_v, losses[3] = [loss, loss_a, loss_v], dWx, dbx, dWy, dby, dX, dY)"""
    (B, D), C = x.shape, Wx.shape[0]
    out, out_a, out_v, losses = _f32((B, C), x), _f32((B, C), x), _f32((B, C), x), _f32(3, x)
    dWx, dbx, dWy, dby, dX, dY = _f32((C, D), x), _f32(C, x), _f32((C, D), x), _f32(C, x), _f32((B, D), x), _f32((B, D), x)
    ops.fusion_sum_ce_fwd_bwd(x, y, Wx, bx, Wy, by, labels, out, out_a, out_v, losses, dWx, dbx, dWy, dby, dX, dY, _fusion_ws(x, C),
                              inv_batch, bias_scale)
    return out, out_a, out_v, losses, dWx, dbx, dWy, dby, dX, dY


@_op("fusion_sum_fwd(Tensor x, Tensor y, Tensor Wx, Tensor bx, Tensor Wy, Tensor by, float bias_scale=1.0) -> (Tensor, Tensor, Tensor)")
def fusion_sum_fwd(x, y, Wx, bx, Wy, by, bias_scale=1.0):
    """(out, out_a, out_v)"""
    (B, _D), C = x.shape, Wx.shape[0]
    out, out_a, out_v = _f32((B, C), x), _f32((B, C), x), _f32((B, C), x)
    ops.fusion_sum_fwd(x, y, Wx, bx, Wy, by, out, out_a, out_v, bias_scale)
    return out, out_a, out_v


@_op("fusion_sum_bwd(Tensor x, Tensor y, Tensor Wx, Tensor Wy, Tensor dlogits, float scale=1.0) -> "
     "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def fusion_sum_bwd(x, y, Wx, Wy, dlogits, scale=1.0):
    """(dWx, dbx, dWy, dby, dX, dY)"""
    (B, D), C = x.shape, Wx.shape[0]
    dWx, dbx, dWy, dby, dX, dY = _f32((C, D), x), _f32(C, x), _f32((C, D), x), _f32(C, x), _f32((B, D), x), _f32((B, D), x)
    ops.fusion_sum_bwd(x, y, Wx, Wy, dlogits, dWx, dbx, dWy, dby, dX, dY, _fusion_ws(x, C), scale)
    return dWx, dbx, dWy, dby, dX, dY


@_op("fusion_film_ce_fwd_bwd(Tensor film, Tensor t, Tensor W, Tensor b, Tensor Wout, Tensor bout, Tensor labels, float inv_batch) -> "
     "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def fusion_film_ce_fwd_bwd(film, t, W, b, Wout, bout, labels, inv_batch):
    """(out, h (B, 2D), z, loss[1], dW, db, dWout, dbout, dfilm, dt)"""
    (B, D), C = film.shape, Wout.shape[0]
    out, h, z, loss = _f32((B, C), t), _f32((B, 2 * D), t), _f32((B, D), t), _f32(1, t)
    dW, db, dWout, dbout, dfilm, dt = _f32((2 * D, D), t), _f32(2 * D, t), _f32((C, D), t), _f32(C, t), _f32((B, D), t), _f32((B, D), t)
    ops.fusion_film_ce_fwd_bwd(film, t, W, b, Wout, bout, labels, out, h, z, loss, dW, db, dWout, dbout, dfilm, dt, _fusion_ws(t, C),
                               inv_batch)
    return out, h, z, loss, dW, db, dWout, dbout, dfilm, dt


@_op("fusion_film_fwd(Tensor film, Tensor t, Tensor W, Tensor b, Tensor Wout, Tensor bout) -> (Tensor, Tensor, Tensor)")
def fusion_film_fwd(film, t, W, b, Wout, bout):
    """(out, h (B, 2D), z)"""
    (B, D), C = film.shape, Wout.shape[0]
    out, h, z = _f32((B, C), t), _f32((B, 2 * D), t), _f32((B, D), t)
    ops.fusion_film_fwd(film, t, W, b, Wout, bout, out, h, z)
    return out, h, z


@_op("fusion_film_bwd(Tensor film, Tensor t, Tensor W, Tensor Wout, Tensor h, Tensor z, Tensor dlogits, float scale=1.0) -> "
     "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def fusion_film_bwd(film, t, W, Wout, h, z, dlogits, scale=1.0):
    """(dW, db, dWout, dbout, dfilm, dt)"""
    (B, D), C = film.shape, Wout.shape[0]
    dW, db, dWout, dbout, dfilm, dt = _f32((2 * D, D), t), _f32(2 * D, t), _f32((C, D), t), _f32(C, t), _f32((B, D), t), _f32((B, D), t)
    ops.fusion_film_bwd(film, t, W, Wout, h, z, dlogits, dW, db, dWout, dbout, dfilm, dt, _fusion_ws(t, C), scale)
    return dW, db, dWout, dbout, dfilm, dt


def _gated_grads(x, C):
    B, D = x.shape
    return (_f32((D, D), x), _f32(D, x), _f32((D, D), x), _f32(D, x), _f32((C, D), x), _f32(C, x), _f32((B, D), x), _f32((B, D), x))


@_op("fusion_gated_ce_fwd_bwd(Tensor x, Tensor y, Tensor Wx, Tensor bx, Tensor Wy, Tensor by, Tensor Wout, Tensor bout, Tensor labels, "
     "bool x_gate, float inv_batch) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def fusion_gated_ce_fwd_bwd(x, y, Wx, bx, Wy, by, Wout, bout, labels, x_gate, inv_batch):
    """(out, hx, hy, z, loss[1], dWx, dbx, dWy, dby, dWout, dbout, dX, dY)"""
    (B, D), C = x.shape, Wout.shape[0]
    out, hx, hy, z, loss = _f32((B, C), x), _f32((B, D), x), _f32((B, D), x), _f32((B, D), x), _f32(1, x)
    g = _gated_grads(x, C)
    ops.fusion_gated_ce_fwd_bwd(x, y, Wx, bx, Wy, by, Wout, bout, labels, out, hx, hy, z, loss, *g, _fusion_ws(x, C), x_gate, inv_batch)
    return (out, hx, hy, z, loss) + g


@_op("fusion_gated_fwd(Tensor x, Tensor y, Tensor Wx, Tensor bx, Tensor Wy, Tensor by, Tensor Wout, Tensor bout, bool x_gate=True) -> "
     "(Tensor, Tensor, Tensor, Tensor)")
def fusion_gated_fwd(x, y, Wx, bx, Wy, by, Wout, bout, x_gate=True):
    """(out, hx, hy, z)"""
    (B, D), C = x.shape, Wout.shape[0]
    out, hx, hy, z = _f32((B, C), x), _f32((B, D), x), _f32((B, D), x), _f32((B, D), x)
    ops.fusion_gated_fwd(x, y, Wx, bx, Wy, by, Wout, bout, out, hx, hy, z, x_gate)
    return out, hx, hy, z


@_op("fusion_gated_bwd(Tensor x, Tensor y, Tensor Wx, Tensor Wy, Tensor Wout, Tensor hx, Tensor hy, Tensor z, Tensor dlogits, "
     "bool x_gate=True, float scale=1.0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
def fusion_gated_bwd(x, y, Wx, Wy, Wout, hx, hy, z, dlogits, x_gate=True, scale=1.0):
    """(dWx, dbx, dWy, dby, dWout, dbout, dX, dY)"""
    g = _gated_grads(x, Wout.shape[0])
    ops.fusion_gated_bwd(x, y, Wx, Wy, Wout, hx, hy, z, dlogits, *g, _fusion_ws(x, Wout.shape[0]), x_gate, scale)
    return g


@_op("qmf_head_fwd_bwd(Tensor[] xs, Tensor[] Ws, Tensor[] bs, Tensor labels, Tensor idx, Tensor(a!) correctness, "
     "Tensor(b!) confidence, float w_cml, float w_crl, float inv_batch) -> "
     "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor[], Tensor[], Tensor[])")
def qmf_head_fwd_bwd(xs, Ws, bs, labels, idx, correctness, confidence, w_cml, w_crl, inv_batch):
    """QMF training head (main.py:239-268): (z (M, B, C), out, conf (M, B), ell (M, B), target (M, B), margin (M, B),
    losses [L, CE_m.., rank_m.., CE(out)], [dW_m], [db_m], [dX_m]); the fp64 History (M, n_data) is updated in place."""
    M, (B, D), C = len(xs), xs[0].shape, Ws[0].shape[0]
    x0 = xs[0]
    z, out, losses = _f32((M, B, C), x0), _f32((B, C), x0), _f32(2 * M + 2, x0)
    conf, ell, target, margin = (_f32((M, B), x0) for _ in range(4))
    dWs, dbs, dxs = [_f32((C, D), x0) for _ in range(M)], [_f32(C, x0) for _ in range(M)], [_f32((B, D), x0) for _ in range(M)]
    ops.qmf_head_fwd_bwd(list(xs), list(Ws), list(bs), labels, idx.reshape(-1), correctness, confidence, z, out, conf, ell, target,
                         margin, losses, dWs, dbs, dxs, _f32(ops.qmf_head_ws_elems(B, C, M), x0), w_cml, w_crl, inv_batch)
    return z, out, conf, ell, target, margin, losses, dWs, dbs, dxs


@_op("qmf_head_fwd(Tensor[] xs, Tensor[] Ws, Tensor[] bs) -> (Tensor, Tensor, Tensor)")
def qmf_head_fwd(xs, Ws, bs):
    """(z (M, B, C), out, conf (M, B)) of the QMF heads (valid(), main.py:576-586)"""
    M, (B, _D), C = len(xs), xs[0].shape, Ws[0].shape[0]
    z, out, conf = _f32((M, B, C), xs[0]), _f32((B, C), xs[0]), _f32((M, B), xs[0])
    ops.qmf_head_fwd(list(xs), list(Ws), list(bs), z, out, conf)
    return z, out, conf


@_op("gs_project(Tensor(a!) Pl, Tensor X, Tensor(b!) G, float alpha) -> ()")
def gs_project(Pl, X, G, alpha):
    """GSPlugin.before_update body (utils/utils.py:34-41) on the batch features X (B, D): Pl and G updated in place."""
    D, C = Pl.shape[0], G.shape[0]
    r = _f32(D, X)
    ops.colsum(X, r, 1.0 / X.shape[0])
    ops.gs_project(Pl, r, G, alpha, _f32(ops.gs_ws_elems(D, C), X))


@_op("gs_project_owm(Tensor(a!) Pl, Tensor X, Tensor(b!) G, float alpha) -> ()")
def gs_project_owm(Pl, X, G, alpha):
    """GSPlugin(mode="owm").before_update body on the batch features X (B, D): k = Pl r, s = alpha + r . k, Pl <- Pl - k k^T / s,
    G <- G Pl^T with r = mean(X, 0); Pl and G updated in place."""
    D, C = Pl.shape[0], G.shape[0]
    r = _f32(D, X)
    ops.colsum(X, r, 1.0 / X.shape[0])
    ops.gs_project_owm(Pl, r, G, alpha, _f32(ops.gs_owm_ws_elems(D, C), X))


@_op("sgd_step(Tensor(a!) p, Tensor? g, Tensor(b!) buf, float lr, float momentum, float weight_decay, bool first) -> ()")
def sgd_step(p, g, buf, lr, momentum, weight_decay, first):
    ops.sgd_step(p, g, buf, lr, momentum, weight_decay, first)


@_op("feature_phase(Tensor X, Tensor labels, Tensor(a!) W, Tensor(b!) b, Tensor(c!) buf, Tensor(d!)? Pl, float inv_batch, "
     "bool project, float alpha, float lr, float momentum, float weight_decay, bool first) -> (Tensor, Tensor)")
def feature_phase(X, labels, W, b, buf, Pl, inv_batch, project, alpha, lr, momentum, weight_decay, first):
    """One head-only modality phase on stored features (main.py:432-442): (logits, loss[1]); W, b, the momentum buffer over
    [W | b] and (when `project`) Pl updated in place."""
    B, D = X.shape
    C = W.shape[0]
    logits, loss = _f32((B, C), X), _f32(1, X)
    ops.feature_phase(X, labels, W, b, buf, Pl, logits, loss, _f32(max(ops.feature_ws_elems(B, D, C), 1), X), inv_batch, project, alpha,
                      lr, momentum, weight_decay, first)
    return logits, loss


@_op("eval_head(Tensor[] feats, Tensor W, Tensor b, Tensor labels, Tensor(a!) counts, int mode, float[] alphas, "
     "Tensor? present=None) -> (Tensor, Tensor, Tensor, Tensor)")
def eval_head(feats, W, b, labels, counts, mode, alphas, present=None):
    """One evaluation batch from features to counters with per-sample fusion weights (main.py:65-106, 636-676 per row):
    (logits (M, B, C), fused (B, C), weights (B, M), pred int32 (B, 1 + M)); `counts` accumulated in place."""
    M, B, C = len(feats), feats[0].shape[0], W.shape[0]
    logits, fused, weights = _f32((M, B, C), W), _f32((B, C), W), _f32((B, M), W)
    pred = torch.empty((B, 1 + M), device=W.device, dtype=torch.int32)
    ops.eval_head(list(feats), W, b, labels, counts, logits, mode=mode, alphas=list(alphas), present=present, fused_out=fused,
                  weights_out=weights, pred_out=pred)
    return logits, fused, weights, pred


@_op("average_precision(Tensor scores, Tensor labels) -> Tensor")
def average_precision(scores, labels):
    """Average precision per head and class of one's own scores, class-major fp32 (H, C, N) or (C, N), against integer labels
    (N): float64 (H, C) resp. (C), NaN where a class has no positive (include/mla_hip.h, mla_average_precision)."""
    s = (scores if scores.dim() == 3 else scores.unsqueeze(0)).contiguous()
    H, C, N = s.shape
    lab = labels.clamp(-1, C).to(torch.int32).contiguous()          # every label outside [0, C) is no class, at any width
    ap = torch.empty((H, C), device=s.device, dtype=torch.float64)
    npos = torch.empty(C, device=s.device, dtype=torch.int32)
    ws = torch.empty((H, N), device=s.device, dtype=torch.float64)
    ops.average_precision(s, lab, N, ap, npos, ws)
    return ap if scores.dim() == 3 else ap[0]


@_op("confusion_count(Tensor pred, Tensor labels, int C) -> Tensor")
def confusion_count(pred, labels, C):
    """Confusion counts of one's own predictions, integer (H, N) or (N), against integer labels (N): int32 (H, C, C) resp. (C, C),
    [true][predicted]; rows whose label or prediction lies outside [0, C) are skipped."""
    p = (pred if pred.dim() == 2 else pred.unsqueeze(0)).to(torch.int32).contiguous()
    conf = torch.zeros((p.shape[0], C, C), device=p.device, dtype=torch.int32)
    ops.confusion_count(p, labels.clamp(-1, C).to(torch.int32).contiguous(), p.shape[1], conf)
    return conf if pred.dim() == 2 else conf[0]


@_op("fusion_sweep(Tensor logits, Tensor labels, Tensor grid, Tensor(a!) tp, Tensor(b!) pp, Tensor(c!)? num=None, "
     "Tensor? present=None) -> ()")
def fusion_sweep(logits, labels, grid, tp, pp, num=None, present=None):
    """The fixed-weight fusion of the per-modality logits (M, B, C) at every row of grid (G, M), in one launch: int32 tp (G, C), pp
    (G, C) and num (C) accumulated in place (include/mla_hip.h, mla_fusion_sweep)."""
    ops.fusion_sweep([logits[m] for m in range(logits.shape[0])], labels, grid, tp, pp, num=num, present=present)


@_op("gate_sweep(Tensor logits, Tensor labels, Tensor grid, Tensor(a!) tp, Tensor(b!) pp, Tensor(c!)? num=None, "
     "Tensor? present=None, Tensor(d!)? ent_out=None) -> ()")
def gate_sweep(logits, labels, grid, tp, pp, num=None, present=None, ent_out=None):
    """The gated fusion w_m ~ a_m exp(-beta H_m) of the per-modality logits (M, B, C) at every gate of grid (G, M + 1), in one
    launch: int32 tp (G, C), pp (G, C) and num (C) accumulated in place, ent_out (B, M) written (include/mla_hip.h, mla_gate_sweep)."""
    ops.gate_sweep([logits[m] for m in range(logits.shape[0])], labels, grid, tp, pp, num=num, present=present, ent_out=ent_out)


@_op("eval_head_gated(Tensor[] feats, Tensor W, Tensor b, Tensor labels, Tensor(a!) counts, float[] prior, float beta, "
     "Tensor? present=None) -> (Tensor, Tensor, Tensor, Tensor)")
def eval_head_gated(feats, W, b, labels, counts, prior, beta, present=None):
    """eval_head under the gate (prior, beta): (logits (M, B, C), fused (B, C), weights (B, M), pred int32 (B, 1 + M)); `counts`
    accumulated in place (include/mla_hip.h, mla_eval_head_gated)."""
    M, B, C = len(feats), feats[0].shape[0], W.shape[0]
    logits, fused, weights = _f32((M, B, C), W), _f32((B, C), W), _f32((B, M), W)
    pred = torch.empty((B, 1 + M), device=W.device, dtype=torch.int32)
    ops.eval_head_gated(list(feats), W, b, labels, counts, logits, prior=list(prior), beta=beta, present=present, fused_out=fused,
                        weights_out=weights, pred_out=pred)
    return logits, fused, weights, pred


@_op("gather_rows2(Tensor T0, Tensor T1, Tensor labels, Tensor idx) -> (Tensor, Tensor, Tensor, Tensor)")
def gather_rows2(T0, T1, labels, idx):
    """(out0 (B, D), out1 (B, D), label (B), idx (B, 1)): rows `idx` of two device-resident feature tables and their labels."""
    B, D = idx.numel(), T0.shape[1]
    out0, out1 = _f32((B, D), T0), _f32((B, D), T0)
    lab = torch.empty(B, device=T0.device, dtype=torch.int64)
    oi = torch.empty((B, 1), device=T0.device, dtype=torch.int64)
    ops.gather_rows2(T0, T1, labels, idx.reshape(-1), out0, out1, lab, oi)
    return out0, out1, lab, oi


@_op("adam_step(Tensor(a!) p, Tensor? g, Tensor(b!) m, Tensor(c!) v, float lr, float beta1, float beta2, float eps, "
     "float weight_decay, int step) -> ()")
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    ops.adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step)


# ---- transformer rows (models/m3ae.py:65-179; cav_mae.py:86-113) ------------------------------------------------------------
@_op("layernorm_fwd(Tensor x, Tensor w, Tensor b, float eps=1e-5) -> (Tensor, Tensor, Tensor)")
def layernorm_fwd(x, w, b, eps=1e-5):
    M, D = x.shape
    y, mean, rstd = torch.empty_like(x), _f32(M, x), _f32(M, x)
    ops.layernorm_fwd(x, w, b, y, mean, rstd, M, D, eps)
    return y, mean, rstd


@_op("layernorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor mean, Tensor rstd) -> (Tensor, Tensor, Tensor)")
def layernorm_bwd(dy, x, w, mean, rstd):
    M, D = x.shape
    dx, dw, db = torch.empty_like(x), _f32(D, x), _f32(D, x)
    ops.layernorm_bwd(dy, x, w, mean, rstd, dx, dw, db, _f32(ops.colreduce_ws_elems(M, D), x), M, D)
    return dx, dw, db


@_op("linear_fwd(Tensor x, Tensor w_kn, Tensor? bias=None, Tensor? residual=None, bool gelu=False) -> Tensor")
def linear_fwd(x, w_kn, bias=None, residual=None, gelu=False):
    """y = x @ w_kn (+ bias) (+ residual); gelu=True returns gelu(y) (erf form, m3ae.py:77)."""
    M, K = x.shape
    N = w_kn.shape[1]
    y = _f32((M, N), x)
    yg = _f32((M, N), x) if gelu else None
    ops.linear_fwd(x, w_kn, bias, y, 1, M, K, N, residual=residual, y_gelu=yg)
    return yg if gelu else y


@_op("linear_dgrad(Tensor dy, Tensor w_kn, Tensor? residual=None, Tensor? gelu_src=None) -> Tensor")
def linear_dgrad(dy, w_kn, residual=None, gelu_src=None):
    M, N = dy.shape
    K = w_kn.shape[0]
    dx = _f32((M, K), dy)
    ops.linear_dgrad(dy, w_kn, dx, _f32(w_kn.numel(), dy), 1, M, K, N, residual=residual, gelu_src=gelu_src)
    return dx


@_op("linear_wgrad(Tensor x, Tensor dy) -> Tensor")
def linear_wgrad(x, dy):
    M, K = x.shape
    N = dy.shape[1]
    dw = _f32((K, N), x)
    ops.linear_wgrad(x, dy, dw, _f32(ops.linear_wgrad_ws_bytes(M, K, N) // 4 + 4, x), 1, M, K, N)
    return dw


@_op("linear_fwd_bf16(Tensor x, Tensor w_kn, Tensor? bias=None, Tensor? residual=None, bool gelu=False) -> Tensor")
def linear_fwd_bf16(x, w_kn, bias=None, residual=None, gelu=False):
    """linear_fwd on the single-product bf16 arithmetic (K, N multiples of 64)."""
    M, K = x.shape
    N = w_kn.shape[1]
    y = _f32((M, N), x)
    yg = _f32((M, N), x) if gelu else None
    ops.linear_fwd(x, w_kn, bias, y, 1, M, K, N, residual=residual, y_gelu=yg, wsplit=ops.conv2d_wimage_bf16(w_kn.view(1, 1, K, N), True),
                   bf16=True)
    return yg if gelu else y


@_op("linear_dgrad_bf16(Tensor dy, Tensor w_kn, Tensor? residual=None, Tensor? gelu_src=None) -> Tensor")
def linear_dgrad_bf16(dy, w_kn, residual=None, gelu_src=None):
    M, N = dy.shape
    K = w_kn.shape[0]
    dx = _f32((M, K), dy)
    ops.linear_dgrad(dy, w_kn, dx, None, 1, M, K, N, residual=residual, gelu_src=gelu_src,
                     wsplit=ops.conv2d_wimage_bf16(w_kn.view(1, 1, K, N), False), bf16=True)
    return dx


@_op("linear_wgrad_bf16(Tensor x, Tensor dy) -> Tensor")
def linear_wgrad_bf16(x, dy):
    M, K = x.shape
    N = dy.shape[1]
    dw = _f32((K, N), x)
    ops.linear_wgrad(x, dy, dw, _f32(ops.linear_wgrad_ws_bytes(M, K, N, bf16=True) // 4 + 4, x), 1, M, K, N, bf16=True)
    return dw


@_op("attention_fwd(Tensor qkv, Tensor? pad_mask, int heads) -> (Tensor, Tensor)")
def attention_fwd(qkv, pad_mask, heads):
    """qkv (B, n, 3*D) -> (o (B, n, D), lse (B, heads, n)): softmax(q k^T * hd^-0.5 masked with -1e7) v (m3ae.py:102-125)."""
    B, n, D3 = qkv.shape
    D = D3 // 3
    o, lse = _f32((B, n, D), qkv), _f32((B, heads, n), qkv)
    ops.attention_fwd(qkv, pad_mask, o, lse, B, heads, n, D // heads)
    return o, lse


@_op("attention_bwd(Tensor do, Tensor qkv, Tensor o, Tensor lse, Tensor? pad_mask, int heads) -> Tensor")
def attention_bwd(do, qkv, o, lse, pad_mask, heads):
    B, n, D3 = qkv.shape
    D = D3 // 3
    dqkv = torch.empty_like(qkv)
    ops.attention_bwd(do, qkv, o, lse, pad_mask, dqkv, _f32((B, heads, n), qkv), B, heads, n, D // heads)
    return dqkv


# ---- the same attention on the split-bf16 arithmetic (attention_math "split") ---------------------------------------------------
@_op("attention_fwd_split(Tensor qkv, Tensor? pad_mask, int heads) -> (Tensor, Tensor)")
def attention_fwd_split(qkv, pad_mask, heads):
    B, n, D3 = qkv.shape
    D = D3 // 3
    o, lse = _f32((B, n, D), qkv), _f32((B, heads, n), qkv)
    ops.attention_fwd(qkv, pad_mask, o, lse, B, heads, n, D // heads, math="split")
    return o, lse


@_op("attention_bwd_split(Tensor do, Tensor qkv, Tensor o, Tensor lse, Tensor? pad_mask, int heads) -> Tensor")
def attention_bwd_split(do, qkv, o, lse, pad_mask, heads):
    B, n, D3 = qkv.shape
    D = D3 // 3
    dqkv = torch.empty_like(qkv)
    ops.attention_bwd(do, qkv, o, lse, pad_mask, dqkv, _f32((B, heads, n), qkv), B, heads, n, D // heads, math="split")
    return dqkv


# ---- CREMA-D frame augmentation (dataset/dataset.py:128-153) --------------------------------------------------------
@_op("frames_resample(Tensor frames, Tensor desc, Tensor lut, int T, int out_h=224, int out_w=224) -> Tensor")
def frames_resample(frames, desc, lut, T, out_h=224, out_w=224):
    """Packed uint8 HWC frames (device) + descriptors int64 (N, 8) (host; validated there, then copied to the device) ->
    (N / T, 3, T, out_h, out_w) fp32: crop, bilinear resize, flip, LUT (mla_hip.frames)."""
    desc_host = desc.cpu().contiguous()
    N = desc_host.shape[0]
    if T <= 0 or N % T:
        raise ops.MLAHipError(f"frames_resample: {N} frames are not a whole number of samples of T={T}")
    out = _f32((N // T, 3, T, out_h, out_w), frames)
    ops.frames_resample(frames, desc_host.to(frames.device), desc_host, lut, out, T)
    return out


# ---- CAV-MAE batch feed (dataset/dataset.py:251-256, 281-294, 303-321) ------------------------------------------------
@_op("image_resample(Tensor frames, Tensor desc, Tensor lut, int T, int out_h=224, int out_w=224, int filter=1) -> Tensor")
def image_resample(frames, desc, lut, T, out_h=224, out_w=224, filter=1):
    """Packed uint8 HWC frames (device) + descriptors int64 (N, 12) (host; validated there, then copied to the device) ->
    (N / T, 3, T, out_h, out_w) fp32: crop, bilinear / bicubic resize, window, flip, LUT (mla_hip.cav_feed)."""
    desc_host = desc.cpu().contiguous()
    N = desc_host.shape[0]
    if T <= 0 or N % T:
        raise ops.MLAHipError(f"image_resample: {N} frames are not a whole number of samples of T={T}")
    out = _f32((N // T, 3, T, out_h, out_w), frames)
    ops.image_resample(frames, desc_host.to(frames.device), desc_host, lut, out, T, filter)
    return out


@_op("fbank_augment(Tensor x, Tensor desc, float mean, float std, int seed) -> Tensor")
def fbank_augment(x, desc, mean, std, seed):
    """fbanks fp32 (B, T, F) (device) + descriptors int64 (B, 8) (host; validated there, then copied to the device) -> a new
    (B, T, F): SpecAug masks, normalisation, Philox noise, roll (mla_hip.cav_feed)."""
    desc_host = desc.cpu().contiguous()
    out = torch.empty_like(x)
    ops.fbank_augment(x, out, desc_host.to(x.device), desc_host, mean, std, seed)
    return out


# ---- M3AE / Food-101 train image transform (dataset/dataset.py:401-412) -------------------------------------------------
@_op("image_augment(Tensor frames, Tensor desc, Tensor jitter, Tensor lut, int out_h=256, int out_w=256) -> Tensor")
def image_augment(frames, desc, jitter, lut, out_h=256, out_w=256):
    """Packed uint8 HWC frames (device) + descriptors int64 (N, 12) and jitter descriptors int64 (N, 7) (host; validated there,
    then copied to the device) -> (N, 3, 1, out_h, out_w) fp32: crop, bicubic resize, flip, ColorJitter, LUT (mla_hip.m3ae_feed)."""
    desc_host, jit_host = desc.cpu().contiguous(), jitter.cpu().contiguous()
    N = desc_host.shape[0]
    out = _f32((N, 3, 1, out_h, out_w), frames)
    staging = torch.empty(N * out_h * out_w * 3, dtype=torch.uint8, device=frames.device)
    partials = torch.empty(N * out_h, dtype=torch.int64, device=frames.device)
    ops.image_augment(frames, desc_host.to(frames.device), desc_host, jit_host.to(frames.device), jit_host, lut, out, staging, partials)
    return out


# ---- Modal3Dataset missing-modality masks (dataset/dataset.py:794-801) ---------------------------------------------------
@_op("modal3_assemble(Tensor image_compact, Tensor(a!) spec, Tensor(b!) token, Tensor(c!) pm, Tensor mask_desc, int size=256) -> Tensor")
def modal3_assemble(image_compact, spec, token, pm, mask_desc, size=256):
    """The P transformed images fp32 (P, 3, size, size) (device; P may be 0) + mask descriptors int64 (B, 4) (host; validated
    there, then copied to the device) -> a new (B, 3, size, size): each sample's image or zeros; spec, token and pm rows of
    absent modalities are zeroed in place (mla_hip.modal3_feed)."""
    desc_host = mask_desc.cpu().contiguous()
    out = _f32((desc_host.shape[0], 3, size, size), spec)
    ops.modal3_assemble(image_compact if image_compact.shape[0] else None, spec, token, pm, desc_host.to(spec.device), desc_host, out)
    return out


# ---- rows of a batch: gather, expand, compact-and-sum (Modal3Classifier(..., present=)) ------------------------------------
def _idx_host(idx: torch.Tensor) -> torch.Tensor:
    return idx.cpu().to(torch.int64).reshape(-1).contiguous()


@_op("rows_gather(Tensor src, Tensor idx, int zero_tail_rows=0) -> Tensor")
def rows_gather(src, idx, zero_tail_rows=0):
    """src (B, ...) fp32 or int64 (device) + row indices int64 (P) (host; validated there, then copied to the device) -> a new
    (P + zero_tail_rows, ...): the rows src[idx[j]], then rows of zeros."""
    h = _idx_host(idx)
    out = torch.empty((h.numel() + zero_tail_rows,) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype)
    return ops.rows_gather(src, h.to(src.device), h, out, zero_tail_rows)


@_op("rows_expand(Tensor src, Tensor idx, int fill_row, int rows) -> Tensor")
def rows_expand(src, idx, fill_row, rows):
    """src fp32 (S, ...) (device) + row indices int64 (P) (host) -> a new (rows, ...): out[idx[j]] = src[j], every other row
    src[fill_row]; the per-row source map is built and validated on the host, then copied to the device."""
    m = ops.rows_expand_map(_idx_host(idx), fill_row, rows, src.shape[0])
    out = torch.empty((rows,) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype)
    return ops.rows_expand(src, m.to(src.device), m, out)


@_op("rows_compact_sum(Tensor src, Tensor idx, Tensor absent_idx) -> Tensor")
def rows_compact_sum(src, idx, absent_idx):
    """src fp32 (B, ...) (device) + row indices int64 (P) and (A) (host; validated there, then copied to the device) -> a new
    (P + 1, ...): the rows src[idx[j]], then the fp32 sum of the rows src[absent_idx[a]] in that order."""
    h, a = _idx_host(idx), _idx_host(absent_idx)
    out = torch.empty((h.numel() + 1,) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype)
    return ops.rows_compact_sum(src, h.to(src.device), h, a.to(src.device), a, out)


# ---- Kaldi log-mel filterbank from PCM16 clips (data/extract_fbank.py:8-54) -------------------------------------------------
@_op("wav_fbank(Tensor wav, Tensor desc, int target_length=1024) -> Tensor")
def wav_fbank(wav, desc, target_length=1024):
    """Packed int16 mono 16 kHz clips (device) + clip descriptors int64 (B, 4) (host; validated there, then copied to the device)
    -> a new (B, target_length, 128) fp32: each clip's Kaldi log-mel filterbank, zero rows beyond its frames (mla_hip.wav_feed)."""
    from .wav_feed import device_tables
    desc_host = desc.cpu().contiguous()
    out = _f32((desc_host.shape[0], target_length, 128), wav)
    ops.wav_fbank(wav, desc_host.to(wav.device), desc_host, device_tables(wav.device), out)
    return out


# ---- HBM-resident CREMA-D feed (mla_hip.resident_feed) --------------------------------------------------------------------------
@_op("resident_batch(Tensor frames, Tensor table, Tensor? spec_table, Tensor labels, Tensor order, int T, int pos, int b, int seed, "
     "int epoch, bool train, Tensor lut, int out_h=224, int out_w=224) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
def resident_batch(frames, table, spec_table, labels, order, T, pos, b, seed, epoch, train, lut, out_h=224, out_w=224):
    """Batch slots 0..b-1 from the samples order[pos : pos + b] of a device-resident dataset (every tensor on the device; the frame
    table is read back once for the plan and its checks) -> new (spec (b, 1024, 128) -- (0, 1024, 128) without a spec table --,
    image (b, 3, T, out_h, out_w), label (b,), idx (b, 1), desc (b * T, 8)): the crops drawn, resampled and gathered on the device."""
    plan = ops.resident_plan(table.cpu().contiguous(), T, frames.numel(), out_h, out_w, train)
    i64 = dict(device=frames.device, dtype=torch.int64)
    spec = _f32((b if spec_table is not None else 0, 1024, 128), frames)
    image = _f32((b, 3, T, out_h, out_w), frames)
    label, idx, desc = torch.empty(b, **i64), torch.empty((b, 1), **i64), torch.empty((b * T, 8), **i64)
    ops.resident_batch(frames, table, spec_table, labels, order, T, pos, b, seed, epoch, train, plan, lut, desc, image,
                       spec if spec_table is not None else None, label, idx)
    return spec, image, label, idx, desc
