"""autograd.Function wrappers: how `loss.backward()` (main.py:435, 447, 459) reaches the HIP backward plans.

The reference's step is written against autograd: `a, v = model(...)` must return tensors with history,
`fc_out(a)` a differentiable Linear, `criterion(out, label).backward()` must end with `.grad` populated on the
head and on ONE encoder.  Each Function below is a thin shell over the same launch plans `MLATrainer` drives:

  EncoderFeature   forward  = encoder forward + global pooling  -> (B, D) feature (fresh tensor)
                   backward = encoder.backward_from_pooled(d feature) -> flat gradient buffer -> p.grad views
                   (after a forward on the present rows only, Modal3Classifier(present=): d feature compacted to those rows first)
  HeadLinear       forward  = mla_head_logits; backward = mla_head_bwd (dW, db, dX in one launch pair)
  ConcatHeadLinear forward  = mla_concat_head_fwd; backward = mla_concat_head_bwd (dW, db, every dX_m; joint step)
  SumFusionHead / FiLMHead / GatedFusionHead   forward = mla_fusion_*_fwd; backward = mla_fusion_*_bwd (every parameter gradient
                   of the fusion module and both feature gradients; joint step with an attached fusion, mla_hip.fusion)
  SoftmaxCE        forward  = mla_ce_fwd_bwd (loss + d logits in one launch); backward = scale by the incoming grad

Graph recording is triggered by a private 1-element `anchor` tensor (requires_grad, not a Parameter): the encoder's
62 parameters are NOT autograd inputs, so no AccumulateGrad nodes / gradient copies exist -- the Function installs
the flat-buffer views as `.grad` itself, with autograd's accumulate rule (module.py).  Under `torch.no_grad()`
(evaluation, main.py:520) nothing is recorded and only the forward kernels run.

Data parallel (mla_hip.DataParallel, one process per GPU): HeadLinear.backward scales dW, db and dX by 1/world (the criterion
averaged over the LOCAL batch), so every local gradient -- the encoder's included, through dX -- is a share of the
global-batch mean; it all-reduces the packed (dW|db) before it is published; the encoder gradient all-reduce (SUM) is issued
asynchronously on RCCL's stream and waited for by FusedSGD.step().
"""
from __future__ import annotations

import torch

from . import ops
from .rows import compact_feature_grad


def make_anchor(device) -> torch.Tensor:
    return torch.zeros(1, device=device, dtype=torch.float32, requires_grad=True)


class EncoderFeature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, enc, run, B, D):
        out = torch.empty((B, D), device=anchor.device, dtype=torch.float32)
        run(out)                                             # HIP forward plan; pooled feature written into `out`
        ctx.enc = enc
        ctx.token = enc._fwd_token = object()                # one live forward state per encoder (workspace is reused)
        return out

    @staticmethod
    def backward(ctx, dfeat):
        enc = ctx.enc
        if enc._fwd_token is not ctx.token:
            raise RuntimeError("mla_hip: backward through a stale encoder forward (the activation workspace holds the "
                               "most recent forward only; retain_graph / double backward are not supported)")
        comm = enc.comm        # data parallel: d feature already is this rank's share of the global-batch mean (HeadLinear.backward
        pending = enc.grads_pending()          # scales by 1 / world), so the flat encoder gradient only needs the SUM over ranks
        enc.backward_from_pooled(compact_feature_grad(enc, dfeat.contiguous()), enc._pa)
        if comm is not None and comm.active:
            enc._grad_works = comm.allreduce_flat_async(enc.grad)      # waited for by FusedSGD.step()
            if pending is not None:                                    # accumulation: add the older gradient after the exchange
                comm.wait(enc._grad_works)
                enc._grad_works = []
        enc.publish_grads(pending)
        return None, None, None, None, None


class HeadLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, head, x):
        xd = x.detach().contiguous()
        out = torch.empty((xd.shape[0], head.out_features), device=xd.device, dtype=torch.float32)
        ops.head_logits(xd, head.weight.detach(), head.bias.detach(), out)
        ctx.head, ctx.x = head, xd
        return out

    @staticmethod
    def backward(ctx, dlogits):
        head, x = ctx.head, ctx.x
        comm = head.comm
        active = comm is not None and comm.active
        pending = head.grads_pending()
        dX = torch.empty_like(x)
        ops.head_bwd(x, head.weight.detach(), dlogits.contiguous(), head.weight_grad, head.bias_grad, dX,
                     (1.0 / comm.world) if active else 1.0)
        if active:
            comm.allreduce_small(head.grad)                          # critical path: packed dW|db, one message
        head.publish_grads(pending)
        return None, None, dX


class ConcatHeadLinear(torch.autograd.Function):
    """fc_out(cat(x_1 .. x_M)) of the joint step (fusion_modules.py:22-23, 32-34) on the concatenated-head kernels: the
    concatenation is never formed; backward hands each modality its own dX_m, so ONE `loss.backward()` (main.py:310)
    reaches every encoder's EncoderFeature node."""

    @staticmethod
    def forward(ctx, anchor, head, *xs):
        xd = [x.detach().contiguous() for x in xs]
        B = xd[0].shape[0]
        out = torch.empty((B, head.out_features), device=xd[0].device, dtype=torch.float32)
        out_m = torch.empty((len(xd), B, head.out_features), device=xd[0].device, dtype=torch.float32)
        ops.concat_head_fwd(xd, head.weight.detach(), head.bias.detach(), out, out_m)
        ctx.head, ctx.xs = head, xd
        return out

    @staticmethod
    def backward(ctx, dlogits):
        head, xs = ctx.head, ctx.xs
        comm = head.comm
        active = comm is not None and comm.active
        pending = head.grads_pending()
        dxs = [torch.empty_like(x) for x in xs]
        ops.concat_head_bwd(xs, head.weight.detach(), dlogits.contiguous(), head.weight_grad, head.bias_grad, dxs,
                            (1.0 / comm.world) if active else 1.0)
        if active:
            comm.allreduce_small(head.grad)                          # critical path: packed dW|db, one message
        head.publish_grads(pending)
        return (None, None) + tuple(dxs)


def _fusion_io(fusion, x, y):
    if fusion.comm is not None and fusion.comm.active:
        raise NotImplementedError("data-parallel training with an attached sum / film / gated fusion is not implemented")
    xd, yd = x.detach().contiguous(), y.detach().contiguous()
    f32 = dict(device=xd.device, dtype=torch.float32)
    B, D = xd.shape
    return xd, yd, B, D, fusion.out_features, f32


def _fusion_publish(fusion, run):
    """The backward of an attached fusion module: `run()` overwrites its whole flat gradient; autograd's accumulate rule on top."""
    pending = fusion.grads_pending()
    run()
    fusion.publish_grads(pending)


class SumFusionHead(torch.autograd.Function):
    """fc_x(x) + fc_y(y) (fusion_modules.py:11-13): one `loss.backward()` fills fc_x / fc_y and hands each encoder its feature gradient."""

    @staticmethod
    def forward(ctx, anchor, fusion, x, y):
        xd, yd, B, _D, C, f32 = _fusion_io(fusion, x, y)
        out, out_a, out_v = (torch.empty((B, C), **f32) for _ in range(3))
        w = fusion.p
        ops.fusion_sum_fwd(xd, yd, w["fc_x.weight"], w["fc_x.bias"], w["fc_y.weight"], w["fc_y.bias"], out, out_a, out_v)
        ctx.fusion, ctx.xy = fusion, (xd, yd)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        fusion, (x, y) = ctx.fusion, ctx.xy
        w, g = fusion.p, fusion.g
        dX, dY = torch.empty_like(x), torch.empty_like(y)
        ws = torch.empty(ops.fusion_ws_elems(x.shape[0], x.shape[1], fusion.out_features), device=x.device, dtype=torch.float32)
        _fusion_publish(fusion, lambda: ops.fusion_sum_bwd(x, y, w["fc_x.weight"], w["fc_y.weight"], dlogits.contiguous(), g["fc_x.weight"],
                                                           g["fc_x.bias"], g["fc_y.weight"], g["fc_y.bias"], dX, dY, ws))
        return None, None, dX, dY


class FiLMHead(torch.autograd.Function):
    """fc_out(gamma * t + beta), gamma | beta = fc(film) (fusion_modules.py:53-67); (film, t) = (x, y) under x_film, else (y, x)."""

    @staticmethod
    def forward(ctx, anchor, fusion, x, y):
        xd, yd, B, D, C, f32 = _fusion_io(fusion, x, y)
        film, t = (xd, yd) if fusion.x_film else (yd, xd)
        out, h, z = torch.empty((B, C), **f32), torch.empty((B, 2 * D), **f32), torch.empty((B, D), **f32)
        w = fusion.p
        ops.fusion_film_fwd(film, t, w["fc.weight"], w["fc.bias"], w["fc_out.weight"], w["fc_out.bias"], out, h, z)
        ctx.fusion, ctx.saved = fusion, (film, t, h, z)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        fusion, (film, t, h, z) = ctx.fusion, ctx.saved
        w, g = fusion.p, fusion.g
        dfilm, dt = torch.empty_like(film), torch.empty_like(t)
        ws = torch.empty(ops.fusion_ws_elems(t.shape[0], t.shape[1], fusion.out_features), device=t.device, dtype=torch.float32)
        _fusion_publish(fusion, lambda: ops.fusion_film_bwd(film, t, w["fc.weight"], w["fc_out.weight"], h, z, dlogits.contiguous(),
                                                            g["fc.weight"], g["fc.bias"], g["fc_out.weight"], g["fc_out.bias"], dfilm, dt, ws))
        return (None, None) + ((dfilm, dt) if fusion.x_film else (dt, dfilm))


class GatedFusionHead(torch.autograd.Function):
    """(fc_x(x), fc_y(y), fc_out(gate * other)) (fusion_modules.py:87-98).  Only `out` carries history: the reference's loop never
    differentiates out_x / out_y, and they are returned detached."""

    @staticmethod
    def forward(ctx, anchor, fusion, x, y):
        xd, yd, B, D, C, f32 = _fusion_io(fusion, x, y)
        out, hx, hy, z = torch.empty((B, C), **f32), torch.empty((B, D), **f32), torch.empty((B, D), **f32), torch.empty((B, D), **f32)
        w = fusion.p
        ops.fusion_gated_fwd(xd, yd, w["fc_x.weight"], w["fc_x.bias"], w["fc_y.weight"], w["fc_y.bias"], w["fc_out.weight"],
                             w["fc_out.bias"], out, hx, hy, z, fusion.x_gate)
        ctx.fusion, ctx.saved = fusion, (xd, yd, hx, hy, z)
        ctx.mark_non_differentiable(hx, hy)
        return hx, hy, out

    @staticmethod
    def backward(ctx, _dhx, _dhy, dlogits):
        fusion, (x, y, hx, hy, z) = ctx.fusion, ctx.saved
        w, g = fusion.p, fusion.g
        dX, dY = torch.empty_like(x), torch.empty_like(y)
        ws = torch.empty(ops.fusion_ws_elems(x.shape[0], x.shape[1], fusion.out_features), device=x.device, dtype=torch.float32)
        _fusion_publish(fusion, lambda: ops.fusion_gated_bwd(
            x, y, w["fc_x.weight"], w["fc_y.weight"], w["fc_out.weight"], hx, hy, z, dlogits.contiguous(), g["fc_x.weight"], g["fc_x.bias"],
            g["fc_y.weight"], g["fc_y.bias"], g["fc_out.weight"], g["fc_out.bias"], dX, dY, ws, fusion.x_gate))
        return None, None, dX, dY


class SoftmaxCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        lg = logits.detach().contiguous()
        B, C = lg.shape
        loss = torch.empty(1, device=lg.device, dtype=torch.float32)
        dl = torch.empty_like(lg)
        ws = torch.empty(B, device=lg.device, dtype=torch.float32)
        ops.ce_fwd_bwd(lg, labels, loss, dl, ws, 1.0 / B)
        ctx.dl = dl
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dl = ctx.dl
        ops.scale_by_device_scalar(dl, g.reshape(1).contiguous())   # usually 1.0 (loss.backward()); no host sync
        return dl, None
