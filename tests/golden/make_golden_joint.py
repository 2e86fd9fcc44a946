"""Fixture generator for the joint concat-fusion step (gs_flag false; main.py:164-168, 273-311, 312-417).

Runs only where the reference tree is available (read-only): it imports the reference's unmodified `AVClassifier`
(gs_flag false -> ConcatFusion(1024, 6), basic_model.py:31-34, 72-74) through make_golden.py's helpers, wraps it in
torch.nn.DataParallel, restates the training-loop lines around it (main.py:164, 273-311, 373-408, 416) with
torch.optim.SGD(lr 1e-3, momentum 0.9, weight decay 1e-4), and writes the reference's OUTPUTS as joint_small.npz (data only):

  per case (`normal`: --modulation Normal; `ogm`: OGM, alpha 0.3, epoch inside the modulation window) and step s:
    a, v, out, out_a, out_v, loss, loss_a, loss_v; scores / ratios / coefficients (ogm); the raw head gradient (weight, bias);
    the head weight / bias after optimizer.step(); bn1 running statistics; conv1.weight after the step; abssum and first
    64 entries of the encoder gradients in make_golden.py's keep list (as loss.backward() left them, before any
    modulation); layer4.1.conv2.weight digest;
  `m3ae` (--lorb m3ae, Normal): the reference's MaskedMultimodalAutoencoder text / image encoders (depth 2, vocab 1000)
    and its ConcatFusion(1536, 3) (basic_model.py:152-154, main.py:236-237, 273-311, 416): features, out, out_a, out_v,
    the three losses, the raw head gradient, the head after the step, digests of the encoders after the step;
  the reference's state_dict key list and shapes (DataParallel-prefixed).

    python tests/golden/make_golden_joint.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (imports the reference modules, installs the offline stubs)
from make_golden import O  # noqa: E402

KEEP = ("conv1.weight", "bn1.weight", "bn1.bias", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight",
        "layer2.0.conv1.weight", "layer4.1.conv2.weight", "layer4.1.bn2.weight")


class _JointArgs(G._Args):
    gs_flag = False


def build_reference(seed):
    model = G.AVClassifier(_JointArgs())
    pa, pv = O.make_resnet18_params("audio", seed), O.make_resnet18_params("visual", seed + 1)
    hd = O.make_head_params(1024, 6, seed + 2)
    model.audio_net.load_state_dict(pa)
    model.visual_net.load_state_dict(pv)
    model.fusion_module.fc_out.load_state_dict(hd)
    return torch.nn.DataParallel(model)


def reference_step(model, optimizer, modulation, alpha, spec, image, label, epoch, modulation_starts=0, modulation_ends=50):
    """main.py:164, 273-311, 373-408, 416 (two modalities, concat fusion), restated around the reference modules."""
    softmax, relu, tanh = nn.Softmax(dim=1), nn.ReLU(inplace=True), nn.Tanh()                 # main.py:131-133
    criterion = nn.CrossEntropyLoss()                                                          # :130
    rec = {}
    model.train()
    optimizer.zero_grad()                                                                      # :164
    a, v, out = model(spec.unsqueeze(1).float(), image.float())                                # :273
    weight_size = model.module.fusion_module.fc_out.weight.size(1)                             # :297
    out_v = (torch.mm(v, torch.transpose(model.module.fusion_module.fc_out.weight[:, weight_size // 2:], 0, 1))
             + model.module.fusion_module.fc_out.bias / 2)                                     # :298-299
    out_a = (torch.mm(a, torch.transpose(model.module.fusion_module.fc_out.weight[:, :weight_size // 2], 0, 1))
             + model.module.fusion_module.fc_out.bias / 2)                                     # :301-302
    loss = criterion(out, label)                                                               # :305
    loss_a = criterion(out_a, label)                                                           # :308
    loss_v = criterion(out_v, label)                                                           # :309
    loss.backward()                                                                            # :310
    for k, t in (("a", a), ("v", v), ("out", out), ("out_a", out_a), ("out_v", out_v), ("loss", loss), ("loss_a", loss_a),
                 ("loss_v", loss_v)):
        rec[k] = t.detach().clone()
    fc = model.module.fusion_module.fc_out
    rec["head_grad"], rec["head_bias_grad"] = fc.weight.grad.detach().clone(), fc.bias.grad.detach().clone()
    rec["grads"] = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    if modulation != "Normal":
        score_v = sum([softmax(out_v)[i][label[i]] for i in range(out_v.size(0))])             # :373
        score_a = sum([softmax(out_a)[i][label[i]] for i in range(out_a.size(0))])             # :374
        ratio_v = score_v / score_a                                                            # :376
        ratio_a = 1 / ratio_v                                                                  # :377
        if ratio_v > 1:                                                                        # :379-384
            coeff_v = 1 - tanh(alpha * relu(ratio_v))
            coeff_a = 1
        else:
            coeff_a = 1 - tanh(alpha * relu(ratio_a))
            coeff_v = 1
        rec["scores"] = np.array([float(score_a), float(score_v)], dtype=np.float32)
        rec["ratios"] = np.array([float(ratio_a), float(ratio_v)], dtype=np.float32)
        rec["coeff"] = np.array([float(coeff_a), float(coeff_v)], dtype=np.float32)
        if modulation_starts <= epoch <= modulation_ends:                                      # :392
            for name, parms in model.named_parameters():
                layer = str(name).split('.')[1]                                                # :395
                if 'audio' in layer and len(parms.grad.size()) == 4:                           # :397-402
                    if modulation == 'OGM_GE':
                        parms.grad = parms.grad * coeff_a + \
                            torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                    elif modulation == 'OGM':
                        parms.grad *= coeff_a
                if 'visual' in layer and len(parms.grad.size()) == 4:                          # :404-408
                    if modulation == 'OGM_GE':
                        parms.grad = parms.grad * coeff_v + \
                            torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                    elif modulation == 'OGM':
                        parms.grad *= coeff_v
    optimizer.step()                                                                           # :416
    return rec


def run_case(fx, tag, modulation, alpha, B, spec_hw, T, img_hw, steps, seed):
    print(f"== joint case {tag}: {modulation} alpha={alpha} B={B} spec={spec_hw} T={T} img={img_hw} steps={steps}")
    torch.manual_seed(0)
    model = build_reference(seed)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)       # main.py:749
    for s in range(steps):
        spec = O.portable_normal(seed + 100 + s, (B,) + spec_hw, stream=1, mean=-5.081, std=4.4849)
        image = O.portable_normal(seed + 100 + s, (B, 3, T) + img_hw, stream=2)
        label = O.portable_labels(seed + 100 + s, B, 6)
        rec = reference_step(model, opt, modulation, alpha, spec, image, label, epoch=s)
        p = f"{tag}.s{s}."
        for k in ("a", "v", "out", "out_a", "out_v", "loss", "loss_a", "loss_v", "head_grad", "head_bias_grad"):
            fx[p + k] = rec[k].numpy()
        for k in ("scores", "ratios", "coeff"):
            if k in rec:
                fx[p + k] = rec[k]
        for enc in ("audio_net", "visual_net"):
            for k in KEEP:
                g = rec["grads"][f"module.{enc}.{k}"]
                fx[p + f"grad.{enc}.{k}.abssum"] = np.float64(g.double().abs().sum().item())
                fx[p + f"grad.{enc}.{k}.head"] = g.flatten()[:64].numpy().copy()
        sd = model.module.state_dict()
        fx[p + "head.weight"] = sd["fusion_module.fc_out.weight"].numpy().copy()
        fx[p + "head.bias"] = sd["fusion_module.fc_out.bias"].numpy().copy()
        for enc in ("audio_net", "visual_net"):
            fx[p + f"{enc}.bn1.running_mean"] = sd[f"{enc}.bn1.running_mean"].numpy().copy()
            fx[p + f"{enc}.bn1.running_var"] = sd[f"{enc}.bn1.running_var"].numpy().copy()
            fx[p + f"{enc}.conv1.weight"] = sd[f"{enc}.conv1.weight"].numpy().copy()
            w = sd[f"{enc}.layer4.1.conv2.weight"]
            fx[p + f"{enc}.layer4.1.conv2.weight.sum"] = np.float64(w.double().sum().item())
            fx[p + f"{enc}.layer4.1.conv2.weight.head"] = w.flatten()[:64].numpy().copy()
        # self-consistency of what is recorded: out = out_a + out_v (main.py:297-302 split the bias in halves)
        err = (rec["out"] - rec["out_a"] - rec["out_v"]).abs().max().item()
        assert err < 1e-5, err
    fx[f"{tag}.meta"] = np.array([B, spec_hw[0], spec_hw[1], T, img_hw[0], img_hw[1], steps, seed], dtype=np.int64)
    fx[f"{tag}.modulation"] = np.array(modulation)
    fx[f"{tag}.alpha"] = np.float64(alpha)
    if "state_keys" not in fx:
        sd = model.state_dict()
        fx["state_keys"] = np.array(list(sd.keys()))
        fx["state_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def run_m3ae_case(fx, B=3, depth=2, vocab=1000, n_classes=3, steps=2, seed=63):
    """--lorb m3ae joint step: a, v from the reference encoders (m3ae.py:342-370 restated device-free, as make_golden.py
    does; basic_model.py:182-200: token-mean feature), `_, _, out = fusion_module(a, v)` (main.py:236-237) with the
    reference's ConcatFusion, out_a / out_v (main.py:297-302), CE (main.py:305-309), backward, SGD step."""
    import einops
    import models.m3ae as RM
    from models.fusion_modules import ConcatFusion
    print(f"== joint m3ae case: B={B} depth={depth} vocab={vocab} classes={n_classes} steps={steps}")
    RM.DropPath.forward = lambda self, input, deterministic=False: input           # as make_golden.py (DropPath == identity)
    cfg = dict(model_type=None, emb_dim=768, depth=depth, num_heads=12, mlp_ratio=4, dec_emb_dim=512, dec_depth=1, dec_num_heads=16)

    def build(pseed):
        m = RM.MaskedMultimodalAutoencoder(text_vocab_size=vocab, config_updates=cfg)
        m.load_state_dict(O.make_m3ae_params(pseed, depth=depth, vocab=vocab), strict=True)
        return m

    def fwd_rep(m, image=None, text=None, text_padding_mask=None):                  # m3ae.py:342-370, device-free
        D = m.config.emb_dim
        bs = image.shape[0] if image is not None else text.shape[0]
        xs, pms = [m.cls_token.expand(bs, 1, D)], [torch.zeros((bs, 1))]
        if image is not None:
            xs.append(m.image_embedding(image) + torch.tensor(RM.get_2d_sincos_pos_embed(D, image.shape[1]))
                      + m.get_type_embedding('encoder_image_type_embedding'))
            pms.append(torch.zeros((bs, image.shape[1])))
        if text is not None:
            xs.append(m.text_embedding(text) + torch.tensor(RM.get_1d_sincos_pos_embed(D, text.shape[1]))
                      + m.get_type_embedding('encoder_text_type_embedding'))
            pms.append(text_padding_mask)
        return m.encoder(torch.cat(xs, dim=1), False, torch.cat(pms, dim=1))

    mae_a, mae_v = build(seed), build(seed + 1)
    fusion = ConcatFusion(input_dim=1536, output_dim=n_classes)                     # basic_model.py:152-154
    fusion.fc_out.load_state_dict(O.make_head_params(1536, n_classes, seed + 2))
    opt = torch.optim.SGD(list(mae_a.parameters()) + list(mae_v.parameters()) + list(fusion.parameters()),
                          lr=1e-3, momentum=0.9, weight_decay=1e-4)                  # main.py:749
    crit = nn.CrossEntropyLoss()
    for s in range(steps):
        token = torch.from_numpy(np.minimum((O.portable_uniform(seed + 50 + s, B * 256, 7) * vocab).astype(np.int64), vocab - 1)).view(B, 1, 256)
        pm = torch.zeros(B, 1, 256)
        for b in range(B):
            pm[b, 0, 40 + 37 * b:] = 1.0
        image = O.portable_normal(seed + 50 + s, (B, 3, 256, 256), stream=3)
        label = O.portable_labels(seed + 50 + s, B, n_classes)
        opt.zero_grad()                                                                    # main.py:164
        visual = einops.rearrange(image, 'b c (h p1) (w p2) -> b (h w) (c p1 p2)', p1=16, p2=16)
        a = fwd_rep(mae_a, None, token.squeeze(1), pm.squeeze(1)).mean(dim=1)
        v = fwd_rep(mae_v, visual, None, None).mean(dim=1)
        _, _, out = fusion(a, v)                                                           # main.py:236-237
        weight_size = fusion.fc_out.weight.size(1)
        out_v = torch.mm(v, torch.transpose(fusion.fc_out.weight[:, weight_size // 2:], 0, 1)) + fusion.fc_out.bias / 2
        out_a = torch.mm(a, torch.transpose(fusion.fc_out.weight[:, :weight_size // 2], 0, 1)) + fusion.fc_out.bias / 2
        loss, loss_a, loss_v = crit(out, label), crit(out_a, label), crit(out_v, label)   # main.py:305-309
        loss.backward()                                                                    # :310
        p = f"m3ae.s{s}."
        for k, t in (("a", a), ("v", v), ("out", out), ("out_a", out_a), ("out_v", out_v), ("loss", loss), ("loss_a", loss_a),
                     ("loss_v", loss_v)):
            fx[p + k] = t.detach().numpy().copy()
        fx[p + "head_grad"] = fusion.fc_out.weight.grad.detach().numpy().copy()
        fx[p + "head_bias_grad"] = fusion.fc_out.bias.grad.detach().numpy().copy()
        opt.step()                                                                         # :416
        fx[p + "head.weight"] = fusion.fc_out.weight.detach().numpy().copy()
        fx[p + "head.bias"] = fusion.fc_out.bias.detach().numpy().copy()
        for nm, net in (("mae_a", mae_a), ("mae_v", mae_v)):
            sd = net.state_dict()
            fx[p + f"{nm}.cls_token"] = sd["cls_token"].numpy().copy()
            fx[p + f"{nm}.fc2w.head"] = sd[f"encoder.blocks.{depth - 1}.transformer_mlp.fc2.weight"].flatten()[:64].numpy().copy()
        err = (out - out_a - out_v).abs().max().item()
        assert err < 1e-5, err
    fx["m3ae.meta"] = np.array([B, depth, vocab, n_classes, steps, seed], dtype=np.int64)


if __name__ == "__main__":
    torch.set_num_threads(8)
    fx = {}
    run_case(fx, "normal", "Normal", 0.3, 4, (128, 64), 2, (96, 96), 2, seed=7)
    run_case(fx, "ogm", "OGM", 0.3, 4, (128, 64), 2, (96, 96), 2, seed=7)
    run_m3ae_case(fx)
    path = os.path.join(HERE, "joint_small.npz")
    np.savez_compressed(path, **fx)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
