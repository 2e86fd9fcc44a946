"""conv_math="bf16" end to end: the CREMA-D MLA step and one M3AE encoder against a CPU model of the arithmetic.

CPU model: the oracle's plain torch ResNet-18 forward (oracle.make_resnet18_params, BatchNorm in training mode) with the input and
the weight of every 64..512-channel convolution passed through .bfloat16().float(); the stem stays exact fp32, as on the GPU.

Tolerance.  bf16 rounding turns a one-ulp difference of accumulation order into a 2^-9 relative flip of a later operand, so the
bound cannot be stated in advance; it is measured ON THE REFERENCE SIDE ONLY.  The CPU model runs twice, once with fp32-accumulating
F.conv2d and once with the convolutions in fp64 on the same rounded operands; d = the largest difference of the pooled features and
of the logits between the two.  The GPU is a third summation order: it must lie within 4 d of the fp32 CPU model (features, logits,
step-0 audio loss).  Measured on the CPU for the shapes below (B 4, spectrogram 128 x 64, 2 frames of 96 x 96: those of
mla_small_intended.npz): see D_MEASURED.  The test recomputes d on every run and prints it; D_MEASURED is the record.  On the MI355X
host the run printed d = 2.082e-2 and GPU differences of 2.2e-2 (a), 1.4e-2 (v), 1.5e-2 (logits), 3.8e-3 (loss); M3AE d_f = 5.4e-5,
d_g = 9.2e-4 (the host's own summation order moves them) against 5.8e-5 and 8.7e-4 on the GPU.

The M3AE encoder (depth 1, vocabulary 64) follows the same rule with its Linears: forward hi(x) hi(w)^T + b, backward
dx = hi(dy) hi(w), dw = hi(dy)^T hi(x) (fp32 or fp64 accumulation), everything else fp32; d_f over the features, d_g over the
gradients, each tensor's largest difference relative to that tensor's largest magnitude."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from test_step_gpu import build, inputs  # noqa: E402

# d of the CPU model, fp32-accumulating against fp64 convolutions / Linears, measured on the CPU (see the module docstring)
D_MEASURED = {"resnet features+logits": 2.08e-2, "m3ae feature": 8.5e-5, "m3ae gradients (relative)": 1.08e-3}
SHAPES = dict(B=4, spec_hw=(128, 64), T=2, img_hw=(96, 96))        # mla_small_intended.npz


def hi(t):
    return t.bfloat16().float()


@contextlib.contextmanager
def rounded_convs(fp64):
    """The oracle's conv2d_fwd with the operands of the 64..512-channel convolutions rounded once to bf16."""
    plain = O.conv2d_fwd

    def conv(x, w, stride, pad):
        if x.shape[1] % 64 != 0:
            return plain(x, w, stride, pad)                                      # the stem: exact
        if fp64:
            return F.conv2d(hi(x).double(), hi(w).double(), None, stride, pad).float()
        return F.conv2d(hi(x), hi(w), None, stride, pad)
    O.conv2d_fwd = conv
    try:
        yield
    finally:
        O.conv2d_fwd = plain


def cpu_model(seed, fp64):
    """(a, v, out_a, loss_a) of step 0: pooled features, audio logits and audio loss on the initial head."""
    pa, pv = O.make_resnet18_params("audio", seed), O.make_resnet18_params("visual", seed + 1)
    hd = O.make_head_params(512, 6, seed + 2)
    spec, image, label = inputs(seed, 0, SHAPES["B"], SHAPES["spec_hw"], SHAPES["T"], SHAPES["img_hw"])
    with rounded_convs(fp64):
        fa, _ = O.resnet18_fwd(pa, spec.unsqueeze(1), "audio", update_running=False)
        fv, _ = O.resnet18_fwd(pv, image, "visual", update_running=False)
    a, v = O.av_pool_fwd(fa, fv, SHAPES["B"])
    out_a, loss_a = O.head_ce_fwd_bwd(a, hd["weight"], hd["bias"], label)[:2]
    out_v = v @ hd["weight"].t() + hd["bias"]
    return {"a": a, "v": v, "out_a": out_a, "loss_a": loss_a.reshape(1), "out_v0": out_v}


def test_bf16_step_against_cpu_model():
    seed = 31
    r32, r64 = cpu_model(seed, False), cpu_model(seed, True)
    d = max((r32[k] - r64[k]).abs().max().item() for k in ("a", "v", "out_a", "out_v0"))
    print(f"bf16 step: d (fp32 vs fp64 accumulation of the CPU model) = {d:.3e}; bound 4 d = {4 * d:.3e}")
    assert d > 0
    model, tr, _ = build(seed, "as_intended", False, "bf16")
    spec, image, label = inputs(seed, 0, SHAPES["B"], SHAPES["spec_hw"], SHAPES["T"], SHAPES["img_hw"])
    losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), 0, 10)
    torch.cuda.synchronize()
    got = {"a": tr.last["a"].cpu(), "v": tr.last["v"].cpu(), "out_a": tr.last["out_a"].cpu(), "loss_a": losses["loss_a"].reshape(1).cpu()}
    errs = {k: (got[k] - r32[k]).abs().max().item() for k in got}
    print("bf16 step: GPU against the fp32 CPU model:", {k: f"{e:.3e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= 4 * d, f"{k}: {e:.3e} exceeds 4 d = {4 * d:.3e}"
    # the mode really rounds: the GPU features differ from the exact-fp32 oracle's by more than the split arithmetic ever does
    # (held to 2e-4 in test_step_gpu.py)
    pa, pv = O.make_resnet18_params("audio", seed), O.make_resnet18_params("visual", seed + 1)
    exact_a = O.av_pool_fwd(O.resnet18_fwd(pa, spec.unsqueeze(1), "audio", update_running=False)[0],
                            O.resnet18_fwd(pv, image, "visual", update_running=False)[0], SHAPES["B"])[0]
    assert (got["a"] - exact_a).abs().max().item() > 1e-3, "bf16 features equal the fp32 ones: nothing was rounded"


def _finite_nonzero(t, name):
    assert torch.isfinite(t).all(), f"{name}: not finite"
    assert t.abs().max().item() > 0, f"{name}: all zero"


def test_bf16_trainers_run():
    """Two MLATrainer steps and one JointTrainer step in bf16: finite losses, every gradient buffer finite and non-zero."""
    from mla_hip import AVClassifier, JointTrainer
    seed = 37
    model, tr, _ = build(seed, "as_intended", False, "bf16")
    for s in range(2):
        spec, image, label = inputs(seed, s, SHAPES["B"], SHAPES["spec_hw"], SHAPES["T"], SHAPES["img_hw"])
        losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), s, 10)
        torch.cuda.synchronize()
        for k, v in losses.items():
            assert torch.isfinite(v).all(), f"step {s}: loss {k} = {v}"
        for nm, enc in (("audio", model.audio_net), ("visual", model.visual_net)):
            assert enc.conv_math == "bf16"
            for k in enc.layout:
                _finite_nonzero(enc.g[k], f"step {s} {nm} {k}")
    tr.join()

    class Args:
        fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
    jm = AVClassifier(Args(), seed=0, conv_math="bf16")
    jt = JointTrainer(jm, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    spec, image, label = inputs(seed, 0, SHAPES["B"], SHAPES["spec_hw"], SHAPES["T"], SHAPES["img_hw"])
    jl = jt.train_step(spec.cuda(), image.cuda(), label.cuda(), 0)
    torch.cuda.synchronize()
    for k, v in jl.items():
        assert torch.isfinite(v).all(), f"joint loss {k} = {v}"
    for nm, enc in (("audio", jm.audio_net), ("visual", jm.visual_net)):
        for k in enc.layout:
            _finite_nonzero(enc.g[k], f"joint {nm} {k}")


def test_bf16_protocol_path_equals_fused_trainer():
    """Step 0 through the verbatim reference loop equals MLATrainer.train_step in bf16, under the tolerances of
    test_protocol_gpu.py::test_protocol_path_equals_fused_trainer (loss 1e-6; head, encoder parameters, running statistics 1e-6).
    The protocol model is wrapped in mla_hip.DataParallel (build_protocol), so this is also the data-parallel wrapper's run in bf16."""
    import mla_hip
    from test_protocol_gpu import Args, build_protocol, reference_loop_body
    from test_protocol_gpu import inputs as pinputs
    from util import assert_close
    seed, B = 53, 4
    model, optimizer, gs_plugin = build_protocol(seed, "as_intended", "bf16")
    criterion = mla_hip.CrossEntropyLoss()
    ref_model = build_protocol(seed, "as_intended", "bf16")[0].module
    tr = mla_hip.MLATrainer(ref_model, lr=1e-3, momentum=0.9, weight_decay=1e-4, gs_mode="as_intended")
    model.train()
    spec, image, label = pinputs(seed, 0, B, (128, 64), 2, (64, 64))
    rec = {}
    optimizer.zero_grad()
    reference_loop_body(Args(), model, optimizer, gs_plugin, criterion, spec, image, label, 0, 10, 0.55, rec, False)
    losses = tr.train_step(spec, image, label, 0, 10)
    torch.cuda.synchronize()
    tr.join()
    assert abs(rec["loss"] - losses["loss"].item()) < 1e-6
    assert isinstance(model, mla_hip.DataParallel)
    m = model.module
    assert m.audio_net.conv_math == "bf16"
    assert_close(m.fusion_module.fc_out.flat, ref_model.fusion_module.fc_out.flat, atol=1e-6, name="head")
    for a, b in ((m.audio_net, ref_model.audio_net), (m.visual_net, ref_model.visual_net)):
        assert_close(a.flat, b.flat, atol=1e-6, name="encoder parameters")
        assert_close(a.running, b.running, atol=1e-6, name="BN running statistics")


def test_bf16_evaluator_runs():
    """Evaluator (eval-mode BatchNorm on running statistics, weight images rebuilt once) under conv_math="bf16": finite logits, every
    sample counted, and not the split arithmetic's logits."""
    from mla_hip import Evaluator
    from test_eval_gpu import _model
    B = 4
    spec = O.portable_normal(80, (B, 128, 64), stream=1, mean=-5.081, std=4.4849).cuda()
    image = O.portable_normal(80, (B, 3, 2, 96, 96), stream=2).cuda()
    label = O.portable_labels(80, B, 6).cuda()
    outs = {}
    for math in ("bf16", "split"):
        ev = Evaluator(_model(71, math), dynamic=True, av_alpha=0.5)
        o = ev.update(spec, image, label)
        torch.cuda.synchronize()
        outs[math] = [t.clone() for t in o[:2]]
        assert all(torch.isfinite(t).all() for t in outs[math])
        assert int(ev.counts.cpu()[:6].sum()) == B
    assert (outs["bf16"][0] - outs["split"][0]).abs().max().item() > 1e-4


# ---- M3AE -----------------------------------------------------------------------------------------------------------------------
class _Bf16Linear(torch.autograd.Function):
    """y = hi(x) hi(w)^T + b; dx = hi(dy) hi(w); dw = hi(dy)^T hi(x); db = column sums of dy (fp32).  acc: accumulation dtype."""
    @staticmethod
    def forward(ctx, x, w, b, acc):
        ctx.save_for_backward(x, w)
        ctx.acc = acc
        y = (hi(x).to(acc) @ hi(w).to(acc).t()).float()
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        acc = ctx.acc
        g = hi(dy).to(acc)
        dx = (g @ hi(w).to(acc)).float()
        dw = (g.reshape(-1, g.shape[-1]).t() @ hi(x).to(acc).reshape(-1, x.shape[-1])).float()
        return dx, dw, dy.reshape(-1, dy.shape[-1]).sum(0), None


class _FProxy:
    """torch.nn.functional with `linear` replaced (for the oracle's module-level F)."""
    def __init__(self, acc):
        self.acc = acc

    def linear(self, x, w, b=None):
        return _Bf16Linear.apply(x, w, b, self.acc)

    def __getattr__(self, name):
        return getattr(F, name)


def m3ae_cpu(p, img, dfeat, acc):
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    plain = O.F
    O.F = _FProxy(acc)
    try:
        feat = O.m3ae_feature(leaves, image=img)
        feat.backward(dfeat)
    finally:
        O.F = plain
    return feat.detach(), {k: v.grad for k, v in leaves.items() if v.grad is not None}


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def test_bf16_m3ae_encoder_against_cpu_model():
    from mla_hip import M3AEEncoder
    depth, vocab, B, seed = 1, 64, 2, 77
    p = O.make_m3ae_params(seed, depth=depth, vocab=vocab)
    img = O.portable_normal(seed, (B, 3, 256, 256), stream=7)
    dfeat = O.portable_normal(seed, (B, 768), stream=9)
    f32, g32 = m3ae_cpu(p, img, dfeat, torch.float32)
    f64, g64 = m3ae_cpu(p, img, dfeat, torch.float64)
    d_f = (f32 - f64).abs().max().item()
    d_g = max(_rel(g32[k], g64[k]) for k in g32)
    print(f"bf16 m3ae: d_f = {d_f:.3e}, d_g (relative to each tensor's largest gradient) = {d_g:.3e}")
    assert d_f > 0 and d_g > 0
    enc = M3AEEncoder("image", depth=depth, text_vocab_size=vocab, seed=0, conv_math="bf16")
    enc.load_state_dict(p)
    feat = enc.forward(img.cuda())
    enc.backward_from_pooled(dfeat.cuda())
    torch.cuda.synchronize()
    got = enc.grads_as_reference()
    e_f = (feat.cpu() - f32).abs().max().item()
    e_g = {k: _rel(got[k].cpu().reshape(g32[k].shape), g32[k]) for k in g32}
    worst = max(e_g, key=e_g.get)
    print(f"bf16 m3ae: GPU against the fp32 CPU model: feature {e_f:.3e}; gradients, worst {worst} {e_g[worst]:.3e}")
    assert set(got) == set(g32)
    assert e_f <= 4 * d_f, f"feature: {e_f:.3e} exceeds 4 d_f = {4 * d_f:.3e}"
    for k, e in e_g.items():
        assert e <= 4 * d_g, f"gradient {k}: {e:.3e} exceeds 4 d_g = {4 * d_g:.3e}"
