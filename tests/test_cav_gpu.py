"""`--lorb large`: the visual CAV-MAE encoder, CAVClassifier and one MLA iteration under Adam (--cav_opti) and under SGD, HIP vs
the CPU restatement in tests/cav_model.py.

PARITY UNPINNED against the reference binary, like the audio kind (test_m3ae_gpu.py::test_cavmae_audio_encoder_vs_oracle):
timm==0.4.5 (Attention / Mlp) is neither vendored nor installed; tests/cav_model.py restates cav_mae.py plus timm 0.4.5's
published definitions, and these tests pin the HIP path to that restatement.

Depth 2 (one blocks_v block with norm1 / norm2 + the shared blocks_u block with norm1_v / norm2_v), D 768, 12 heads, B 2, audio
(2, 1024, 128), image (2, 3, 224, 224).  Tolerances are the audio kind's of test_m3ae_gpu.py: encoder feature 2e-5 (+2e-5
relative), every gradient relL2 < 1e-4; step level features / logits / losses / raw head gradients 2e-4 absolute, encoder
gradients relL2 < 2e-4, the projected head gradient against an fp64 re-evaluation on the GPU's own inputs within 20x the fp32
CPU evaluation's error + 1e-4.  conv_math "bf16": d = fp32-accumulating against fp64-accumulating CPU model on bf16-rounded
operands, the GPU within 4 d of the fp32 one (the scheme of test_bf16_step_gpu.py on tests/bf16_model.py's rounding).

Updated parameters under Adam.  The first Adam step moves an element by lr * g / (|g| + eps): about lr * sign(g), so an element
whose gradient is smaller than the gradient's own error is ill-conditioned (2 lr apart for a flipped sign).  As for the
projection, the map is therefore re-evaluated on the GPU's own inputs: CPU torch.optim.Adam with the reference's two groups,
fed the gradients the GPU produced, must reproduce the GPU's updated parameters to 1e-6 (head, two steps; each encoder, one) --
the gradients themselves are held to the restatement above.  Against the restatement's own updated parameters the comparison is
direct on the well-conditioned elements: those where g' = g + wd p, the quantity Adam divides, agrees within 1 % between the GPU and
the restatement (g alone is not enough: where g nearly cancels wd p, 1 % of g is many times g').  There the step
lr g' / (|g'| + eps) differs by at most lr * 0.01 |g'| eps / (|g'| + eps)^2 <= 0.25 % of lr; bound used: 2 % of lr.  These elements
must be at least half of each sampled tensor."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import cav_model as C  # noqa: E402
from oracle import mla_oracle as O  # noqa: E402
from util import assert_close  # noqa: E402

DEPTH, B, LR = 2, 2, 1e-3


class Args:
    fusion_method, dataset, gs_flag, modulation, lorb = "concat", "CREMAD", True, "Normal", "large"


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu().reshape(got.shape)
    return (torch.linalg.norm(got - want) / torch.linalg.norm(want).clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def case():
    """Parameters, one batch and the restatement's results, computed once and never modified."""
    seed = 31
    pa, pv, hd = O.make_cavmae_audio_params(seed, depth=DEPTH), C.make_visual_params(seed + 1, depth=DEPTH), O.make_head_params(768, 6, seed + 2)
    spec = O.portable_normal(seed, (B, 1024, 128), stream=1, mean=-5.081, std=4.4849)
    image = O.portable_normal(seed, (B, 3, 224, 224), stream=2)
    label = O.portable_labels(seed, B, 6)
    ref = {}
    for opt in ("adam", "sgd"):
        st = C.CavState(pa, pv, hd, LR, opt)
        ref[opt] = C.mla_iteration(st, spec, image, label, 0, 10)
        ref[opt]["params"] = {k: v.detach().clone() for k, v in st.p.items()}
    return dict(pa=pa, pv=pv, hd=hd, spec=spec, image=image, label=label, ref=ref)


def state_dict_of(case):
    sd = {f"mae_a.{k}": v for k, v in case["pa"].items()}
    sd.update({f"mae_v.{k}": v for k, v in case["pv"].items()})
    sd.update({f"fusion_module.fc_out.{k}": v for k, v in case["hd"].items()})
    return sd


def build(case, **kw):
    from mla_hip import CAVClassifier
    model = CAVClassifier(Args(), depth=DEPTH, seed=0, **kw)
    model.load_state_dict(state_dict_of(case))
    return model


# ---- the encoder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv_math", ["f32", "split"])
def test_cav_visual_encoder_vs_restatement(case, conv_math):
    from mla_hip import M3AEEncoder
    p, image = case["pv"], case["image"]
    enc = M3AEEncoder("cav_visual", depth=DEPTH, seed=0, conv_math=conv_math)
    enc.load_state_dict(p)
    sd = enc.state_dict()
    assert list(sd) == C.branch_param_names("v", DEPTH) and all(torch.equal(sd[k].cpu(), p[k]) for k in p), "state_dict round trip"
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    feat_ref = C.visual_feature(leaves, image)
    feat = enc.forward(image.cuda())
    assert_close(feat, feat_ref.detach(), atol=2e-5, rtol=2e-5, name="visual feature")
    dfeat = O.portable_normal(7, (B, 768), stream=3)
    feat_ref.backward(dfeat)
    enc.backward_from_pooled(dfeat.cuda())
    torch.cuda.synchronize()
    got = enc.grads_as_reference()
    assert set(got) == {k for k, v in leaves.items() if v.grad is not None} == set(p)
    for k, g in got.items():
        assert g.shape == p[k].shape, k
        err = rel_l2(g, leaves[k].grad)
        assert err < 1e-4, (k, err)


def test_cav_visual_encoder_bf16_against_cpu_model(case):
    from mla_hip import M3AEEncoder
    from test_bf16_step_gpu import _Bf16Linear
    p, image = case["pv"], case["image"]
    dfeat = O.portable_normal(7, (B, 768), stream=3)

    def cpu(acc):
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        feat = C.visual_feature(leaves, image, linear=lambda x, w, b=None: _Bf16Linear.apply(x, w, b, acc))
        feat.backward(dfeat)
        return feat.detach(), {k: v.grad for k, v in leaves.items()}
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    (f32, g32), (f64, g64) = cpu(torch.float32), cpu(torch.float64)
    d_f = (f32 - f64).abs().max().item()
    d_g = max(rel(g32[k], g64[k]) for k in g32)
    print(f"bf16 cav_visual: d_f = {d_f:.3e}, d_g (relative to each tensor's largest gradient) = {d_g:.3e}")
    assert d_f > 0 and d_g > 0
    enc = M3AEEncoder("cav_visual", depth=DEPTH, seed=0, conv_math="bf16")
    enc.load_state_dict(p)
    feat = enc.forward(image.cuda())
    enc.backward_from_pooled(dfeat.cuda())
    torch.cuda.synchronize()
    got = enc.grads_as_reference()
    e_f = (feat.cpu() - f32).abs().max().item()
    e_g = {k: rel(got[k].cpu().reshape(g32[k].shape), g32[k]) for k in g32}
    worst = max(e_g, key=e_g.get)
    print(f"bf16 cav_visual: GPU against the fp32 CPU model: feature {e_f:.3e}; gradients, worst {worst} {e_g[worst]:.3e}")
    assert e_f <= 4 * d_f, f"feature: {e_f:.3e} exceeds 4 d_f = {4 * d_f:.3e}"
    for k, e in e_g.items():
        assert e <= 4 * d_g, f"gradient {k}: {e:.3e} exceeds 4 d_g = {4 * d_g:.3e}"


def test_cav_visual_patch_weight_layout(case):
    """A reference-shaped (D, 3, 16, 16) conv weight through load_state_dict: the embedding the kernels form must be F.conv2d's.
    Every (c, ph, pw) position of the weight carries a different value, so a permuted view gives another embedding; the
    parameter is a view of the flat buffer, not a copy."""
    from mla_hip import M3AEEncoder
    p, image = case["pv"], case["image"]
    enc = M3AEEncoder("cav_visual", depth=DEPTH, seed=0, conv_math="f32")
    w = enc.patch_embed_v.proj.weight
    assert w.shape == (768, 3, 16, 16) and w.untyped_storage().data_ptr() == enc.flat.untyped_storage().data_ptr()
    enc.load_state_dict(p)
    assert torch.equal(enc.p["patch_embed_v.proj.weight"].cpu(), p["patch_embed_v.proj.weight"].flatten(1).t())   # [(c, ph, pw)][D]
    enc.forward(image.cuda())
    torch.cuda.synchronize()
    want = C.visual_embed(p, image)
    assert_close(enc._ws["x0"].view(B, 196, 768), want, atol=2e-5, rtol=2e-5, name="patch embedding + pos + modality")
    wrong = dict(p)
    wrong["patch_embed_v.proj.weight"] = p["patch_embed_v.proj.weight"].permute(0, 1, 3, 2).contiguous()
    assert (C.visual_embed(wrong, image) - want).abs().max().item() > 0.1, "the case must tell (ph, pw) from (pw, ph)"


# ---- the classifier ---------------------------------------------------------------------------------------------------------------
def test_cav_classifier_keys_and_checkpoints(case, tmp_path):
    from mla_hip import CAVClassifier
    model = build(case)
    assert list(model.state_dict()) == C.classifier_keys(DEPTH)
    # CAVMAEFT checkpoints: every key of the materialised branch plus keys of the other branch / unused norms, which are ignored
    extra_a = {"patch_embed_v.proj.weight": torch.zeros(768, 3, 16, 16), "blocks_v.0.attn.qkv.weight": torch.zeros(2304, 768),
               "blocks_u.0.norm1.weight": torch.ones(768), "norm_v.bias": torch.zeros(768)}
    extra_v = {"patch_embed_a.proj.weight": torch.zeros(768, 1, 16, 16), "pos_embed_a": torch.zeros(1, 512, 768),
               "blocks_u.0.norm1_a.weight": torch.ones(768), "norm_a.weight": torch.ones(768)}
    pa2, pv2 = O.make_cavmae_audio_params(77, depth=DEPTH), C.make_visual_params(78, depth=DEPTH)
    fa, fv = os.path.join(tmp_path, "cavmae-audio.pth"), os.path.join(tmp_path, "cavmae-visual.pth")
    torch.save({**pa2, **extra_a}, fa)
    torch.save({**pv2, **extra_v}, fv)
    m2 = CAVClassifier(Args(), depth=DEPTH, seed=0, audio_ckpt=fa, visual_ckpt=fv)
    sd = m2.state_dict()
    assert list(sd) == C.classifier_keys(DEPTH)
    assert all(torch.equal(sd["mae_a." + k].cpu(), v) for k, v in pa2.items())
    assert all(torch.equal(sd["mae_v." + k].cpu(), v) for k, v in pv2.items())
    m3 = CAVClassifier(Args(), depth=DEPTH, seed=0, visual_ckpt=fv)              # None keeps the seeded initialisation
    m4 = CAVClassifier(Args(), depth=DEPTH, seed=0)
    assert torch.equal(m3.mae_a.flat, m4.mae_a.flat) and not torch.equal(m3.mae_v.flat, m4.mae_v.flat)


class RecordingOptimizer:
    """The optimiser the verbatim loop drives, noting the head's gradients as each step() finds them."""

    def __init__(self, inner, head):
        self.inner, self.head, self.head_grads = inner, head, []

    def step(self):
        self.head_grads.append((self.head.weight.grad.detach().cpu().clone(), self.head.bias.grad.detach().cpu().clone()))
        self.inner.step()

    def zero_grad(self):
        self.inner.zero_grad()


def protocol_iteration(model, optimizer, spec, image, label):
    """main.py:419-476 for args.lorb == 'large', verbatim, on the protocol objects."""
    import mla_hip

    class args:
        lorb, modal3 = "large", False
    gs_plugin = mla_hip.GSPlugin()
    criterion = mla_hip.CrossEntropyLoss()
    batch_step, len_dataloader = 0, 10
    model.train()
    optimizer.zero_grad()
    if args.lorb == "large":
        a, v = model(spec, image)
    out_a = model.module.fusion_module.fc_out(a)

    loss_a = criterion(out_a, label)
    loss_a.backward()

    gs_plugin.before_update(model.module.fusion_module.fc_out, a,
                            batch_step, len_dataloader, gs_plugin.exp_count)
    optimizer.step()
    optimizer.zero_grad()

    gs_plugin.exp_count += 1

    out_v = model.module.fusion_module.fc_out(v)

    loss_v = criterion(out_v, label)
    loss_v.backward()

    gs_plugin.before_update(model.module.fusion_module.fc_out, v,
                            batch_step, len_dataloader, gs_plugin.exp_count)
    optimizer.step()
    optimizer.zero_grad()

    gs_plugin.exp_count += 1

    for n, p in model.named_parameters():
        if p.grad != None:
            del p.grad
    torch.cuda.synchronize()
    return dict(out_a=out_a.detach(), out_v=out_v.detach(), loss_a=loss_a.detach(), loss_v=loss_v.detach(), feat_a=a.detach(), feat_v=v.detach())


SAMPLE = ["mae_a.patch_embed_a.proj.weight", "mae_a.pos_embed_a", "mae_a.blocks_a.0.attn.qkv.weight", "mae_a.blocks_u.0.norm1_a.weight",
          "mae_a.blocks_u.0.mlp.fc2.bias", "mae_a.norm_a.bias", "mae_v.patch_embed_v.proj.weight", "mae_v.modality_v",
          "mae_v.blocks_v.0.mlp.fc1.weight", "mae_v.blocks_u.0.norm2_v.bias", "mae_v.blocks_u.0.attn.proj.weight", "mae_v.norm_v.weight"]


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_cav_mla_iteration(case, optimizer):
    """One full MLA iteration (a then v): MLATrainer == the verbatim protocol loop == the CPU restatement."""
    import mla_hip
    from mla_hip import MLATrainer, cav_param_groups
    ref, sd0 = case["ref"][optimizer], state_dict_of(case)
    spec, image, label = case["spec"].cuda(), case["image"].cuda(), case["label"].cuda()
    # ---- fused trainer
    model = build(case, conv_math="f32")
    if optimizer == "adam":
        tr = MLATrainer(model, optimizer="adam", betas=(0.95, 0.999), weight_decay=5e-7, param_groups=cav_param_groups(model, LR))
    else:
        tr = MLATrainer(model, lr=LR)
    tr.keep_debug = True
    losses = tr.train_step(spec, image, label, 0, 10)
    tr.join()
    torch.cuda.synchronize()
    assert set(losses) == {"loss", "loss_a", "loss_v"} and tr.gs_plugin.exp_count == 2
    for nm in ("a", "v"):
        assert_close(tr.last[nm], ref["feat_" + nm], atol=2e-4, name=f"feat {nm}")
        assert_close(tr.last["out_" + nm], ref["out_" + nm], atol=2e-4, name=f"logits {nm}")
        assert_close(losses["loss_" + nm].reshape(()), ref["loss_" + nm], atol=2e-4, name=f"loss {nm}")
        assert_close(tr.last[f"head_grad_{nm}_raw"], ref[f"head_grad_{nm}_raw"], atol=2e-4, name=f"raw head grad {nm}")
    assert_close(losses["loss"].reshape(()), ref["loss"], atol=2e-4, name="reported loss (main.py:472)")
    grads = {}
    for nm, enc in (("a", model.mae_a), ("v", model.mae_v)):
        got = {f"mae_{nm}." + k: g for k, g in enc.grads_as_reference().items()}
        assert set(got) == set(ref["grads_" + nm])
        for k, g in got.items():
            assert rel_l2(g, ref["grads_" + nm][k]) < 2e-4, (nm, k)
        grads.update(got)
    # projected head gradient of phase v (the first projection, from Pl = I): the conditioning-aware criterion of test_m3ae_gpu.py
    feat, G0, Pl0 = tr.last["v"].cpu(), tr.last["head_grad_v_raw"].cpu(), tr.last["Pl_before_v"].cpu()
    _, g32 = O.gs_before_update(Pl0, feat, G0, 0, 10, 1, "as_intended")
    _, g64 = O.gs_before_update(Pl0.double(), feat.double(), G0.double(), 0, 10, 1, "as_intended")
    err_ref = (g32.double() - g64).abs().max().item()
    err_hip = (tr.last["head_grad_v"].cpu().double() - g64).abs().max().item()
    assert err_hip <= 20 * err_ref + 1e-4, (err_hip, err_ref)
    after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    # ---- the optimiser step re-evaluated on the GPU's own gradients: CPU torch optimiser over the same groups
    cpu_p = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    cpu_p = {k: cpu_p[k] for k in C.classifier_keys(DEPTH)}
    base, mlp = C.cav_group_names(list(cpu_p))
    if optimizer == "adam":
        topt = torch.optim.Adam([{"params": [cpu_p[n] for n in base], "lr": LR / 10}, {"params": [cpu_p[n] for n in mlp], "lr": LR}],
                                weight_decay=5e-7, betas=(0.95, 0.999))
    else:
        topt = torch.optim.SGD(list(cpu_p.values()), lr=LR, momentum=0.9, weight_decay=1e-4)
    for nm in ("a", "v"):
        logits = tr.last["out_" + nm].cpu()
        cpu_p["fusion_module.fc_out.weight"].grad = tr.last["head_grad_" + nm].cpu().clone()
        cpu_p["fusion_module.fc_out.bias"].grad = (F.softmax(logits, dim=1) - F.one_hot(case["label"], 6).float()).sum(0) / B
        for k, g in grads.items():
            if k.startswith(f"mae_{nm}."):
                cpu_p[k].grad = g.cpu().reshape(cpu_p[k].shape).clone()
        topt.step()
        topt.zero_grad()
    for k in ["fusion_module.fc_out.weight", "fusion_module.fc_out.bias"] + SAMPLE:
        assert_close(after[k], cpu_p[k].detach(), atol=1e-6, name=f"{optimizer} step on the GPU's gradients: {k}")
    # ---- against the restatement's updated parameters, on the well-conditioned elements
    if optimizer == "adam":
        for k in SAMPLE:
            nm = k[4]
            gg, gr = (g + 5e-7 * sd0[k] for g in (grads[k].cpu().reshape(sd0[k].shape), ref["grads_" + nm][k]))
            good = (gg - gr).abs() <= 0.01 * gr.abs()
            assert good.float().mean().item() >= 0.5, (k, good.float().mean().item())
            err = ((after[k] - ref["params"][k]).abs() * good).max().item()
            assert err <= 0.02 * (LR / 10) + 1e-7, (k, err)
    else:
        for k in SAMPLE:
            assert_close(after[k], ref["params"][k], atol=2e-6, name=f"sgd: {k} after the step")
        assert_close(after["fusion_module.fc_out.bias"], ref["params"]["fusion_module.fc_out.bias"], atol=1e-5, name="head bias")
    # ---- the verbatim protocol loop equals the fused trainer
    pm = mla_hip.DataParallel(build(case, conv_math="f32"), device_ids=[0])
    if optimizer == "adam":
        popt = mla_hip.FusedAdam(cav_param_groups(pm, LR), weight_decay=5e-7, betas=(0.95, 0.999))
    else:
        popt = mla_hip.FusedSGD(pm.parameters(), lr=LR, momentum=0.9, weight_decay=1e-4)
    rec = RecordingOptimizer(popt, pm.module.fusion_module.fc_out)
    got = protocol_iteration(pm, rec, spec, image, label)
    for nm in ("a", "v"):
        assert_close(got["feat_" + nm], tr.last[nm], atol=1e-5, name=f"verbatim loop vs trainer: feature {nm}")
        assert_close(got["out_" + nm], tr.last["out_" + nm], atol=1e-5, name=f"verbatim loop vs trainer: logits {nm}")
        assert abs(got["loss_" + nm].item() - losses["loss_" + nm].item()) < 1e-5, nm
    m = pm.module
    for enc_p, enc_t, name in ((m.mae_a, model.mae_a, "audio"), (m.mae_v, model.mae_v, "visual")):
        assert_close(enc_p.flat, enc_t.flat, atol=2e-6, name=f"verbatim loop vs trainer: {name} encoder after the step")
    if optimizer == "adam":
        assert popt.steps == {"SharedHead0": 2, "M3AEEncoder1": 1, "M3AEEncoder2": 1} and tr.optimizer.steps == {"audio": 1, "visual": 1, "head": 2}
        # the head: the two paths' gradients agree like their logits, and the loop's head is the CPU Adam step on the loop's own
        # gradients (sign-like first steps: see the module docstring)
        hw, hb = (case["hd"][k].clone().requires_grad_(True) for k in ("weight", "bias"))
        hopt = torch.optim.Adam([{"params": [hb], "lr": LR / 10}, {"params": [hw], "lr": LR}], weight_decay=5e-7, betas=(0.95, 0.999))
        for nm, (gw, gb) in zip("av", rec.head_grads):
            assert_close(gw, tr.last["head_grad_" + nm], atol=1e-5, name=f"verbatim loop vs trainer: head gradient {nm}")
            hw.grad, hb.grad = gw, gb
            hopt.step()
        assert_close(m.fusion_module.fc_out.weight, hw.detach(), atol=1e-6, name="verbatim loop: head weight after two Adam steps")
        assert_close(m.fusion_module.fc_out.bias, hb.detach(), atol=1e-6, name="verbatim loop: head bias after two Adam steps")
    else:
        assert_close(m.fusion_module.fc_out.flat, model.fusion_module.fc_out.flat, atol=5e-5, name="verbatim loop vs trainer: head")


def test_cav_evaluator_fixed_alpha(case):
    from mla_hip import Evaluator
    model = build(case, conv_math="f32")
    ev = Evaluator(model, dynamic=False, av_alpha=0.5)
    outs = ev.update(case["spec"].cuda(), case["image"].cuda(), case["label"].cuda())
    torch.cuda.synchronize()
    a = O.cavmae_audio_feature(case["pa"], case["spec"])
    v = C.visual_feature(case["pv"], case["image"])
    ref_outs = [F.linear(f, case["hd"]["weight"], case["hd"]["bias"]) for f in (a, v)]
    for o, r, nm in zip(outs, ref_outs, "av"):
        assert_close(o, r, atol=2e-4, name=f"eval logits {nm}")
    _w, counts = O.valid_batch(ref_outs, case["label"], 6, False, [0.5, 0.5])
    assert torch.equal(ev.counts.view(4, 6).cpu().long(), counts)
    # arg-max ties would make the counters depend on rounding: the case has none
    fused = 0.5 * ref_outs[0] + 0.5 * ref_outs[1]
    for t in (fused, *ref_outs):
        top = t.topk(2, dim=1).values
        assert (top[:, 0] - top[:, 1]).min().item() > 1e-2


def test_cav_joint_trainer_runs(case):
    """Built without gs_flag, the large model goes through JointTrainer like M3AEClassifier: Linear(1536, 6) on cat(a, v)
    (basic_model.py:98; main.py:541-542 applies fusion_module outside the model)."""
    from mla_hip import CAVClassifier, JointTrainer

    class J(Args):
        gs_flag = False
    model = CAVClassifier(J(), depth=DEPTH, seed=3, conv_math="f32")
    assert model.fusion_module.fc_out.weight.shape == (6, 1536)
    sd = {k: v for k, v in state_dict_of(case).items() if not k.startswith("fusion_module.")}
    model.load_state_dict(sd, strict=False)
    tr = JointTrainer(model)
    losses = tr.train_step(case["spec"].cuda(), case["image"].cuda(), case["label"].cuda(), 0)
    torch.cuda.synchronize()
    W, b = model.fusion_module.fc_out.weight.detach().cpu(), model.fusion_module.fc_out.bias.detach().cpu()
    assert_close(tr.last["a"], case["ref"]["sgd"]["feat_a"], atol=2e-4, name="joint feature a")
    assert_close(tr.last["v"], case["ref"]["sgd"]["feat_v"], atol=2e-4, name="joint feature v")
    assert torch.isfinite(losses["loss"]).all() and torch.isfinite(W).all() and torch.isfinite(b).all()
