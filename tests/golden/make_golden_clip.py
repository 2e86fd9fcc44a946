"""Fixture generator for the `--clip` model under --gs_flag (models/basic_model.py:278-319; main.py:428-454).

Runs only where the reference tree is available (read-only): it imports the reference's unmodified `CLIPClassifier` and
`GSPlugin` through make_golden.py's stubs, drives main.py:428-454 around them with torch.optim.SGD(lr 1e-3, momentum 0.9,
weight decay 1e-4) and make_golden's `_Wrap` (so that utils/utils.py:32-41 executes, 'as_intended'; the bare fc_out reproduces
the published no-op), asserts that the restatement in tests/clip_model.py agrees with it, and writes the reference's OUTPUTS as
clip_small.npz (data only):

  per gs mode (`intended`, `published`) and step s of 3 (B = 8, D = 512, C = 101, len_dataloader = 5; features from
  clip_model.clip_inputs: portable_normal mean 0.3 std 0.7, .abs()): out_a, out_v, loss_a, loss_v, loss; the Pl digest
  (corner / strided sub / Frobenius norm / trace) after the step;
  after the last step: head bias and its momentum in full; head weight and its momentum in full for `intended`, and every 4th
  column plus the fp64 sum of absolute values for `published` (four full (101, 512) tensors would not fit the size limit of a
  committed fixture);
  meta = [B, D, C, steps, seed, len_dataloader].

    python tests/golden/make_golden_clip.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (imports the reference modules, installs the offline stubs)
from make_golden import O  # noqa: E402
from models.basic_model import CLIPClassifier  # noqa: E402  (reference)
import clip_model as R  # noqa: E402

B, D, C, STEPS, SEED, LDL = 8, 512, 101, 3, 91, 5


class _ClipArgs(G._Args):
    dataset = "Food101"
    clip = True


def reference_step(model, optimizer, gs, spec, image, label, batch_step, len_dataloader, gs_mode):
    """main.py:428-454, 468-472 restated around the imported reference modules."""
    rec = {}
    model.train()
    optimizer.zero_grad()                                                       # main.py:164
    a, v = model(spec, image)                                                   # :429
    fc = model.module.fusion_module.fc_out
    target = G._Wrap(fc) if gs_mode == "as_intended" else fc
    crit = nn.CrossEntropyLoss()
    for name, feat in (("a", a), ("v", v)):
        out = fc(feat)                                                          # :432 / :444
        loss = crit(out, label)
        loss.backward()                                                         # :435 / :447
        rec["out_" + name], rec["loss_" + name] = out.detach().clone(), loss.detach().clone()
        gs.before_update(target, feat, batch_step, len_dataloader, gs.exp_count)        # :437 / :449
        rec["head_grad_" + name] = fc.weight.grad.detach().clone()
        optimizer.step()                                                        # :439 / :451
        optimizer.zero_grad()
        gs.exp_count += 1
    for _n, p in model.named_parameters():                                      # :468-470
        if p.grad is not None:
            del p.grad
    rec["loss"] = rec["loss_a"] * 0.55 + rec["loss_v"] * 0.45                   # :472 (Q8)
    return rec


def run_mode(fx, tag, gs_mode):
    print(f"== clip case {tag}: B={B} D={D} C={C} steps={STEPS} gs={gs_mode}")
    torch.manual_seed(0)
    model = CLIPClassifier(_ClipArgs())
    hd = O.make_head_params(D, C, SEED + 2)
    model.fusion_module.fc_out.load_state_dict(hd)
    assert list(model.state_dict().keys()) == ["fusion_module.fc_out.weight", "fusion_module.fc_out.bias"]
    model = torch.nn.DataParallel(model)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)       # main.py:749
    gs = G.GSPlugin.__new__(G.GSPlugin)          # ctor needs a GPU (Q3); state set by hand
    gs.Pl = torch.eye(D)
    gs.exp_count = 0
    st = R.ClipState(hd, D)
    for s in range(STEPS):
        tok, img, label = R.clip_inputs(SEED, s, B, D, C)
        ref = reference_step(model, opt, gs, tok, img, label, s, LDL, gs_mode)
        orc = R.clip_gs_step(st, tok, img, label, s, LDL, gs_mode=gs_mode)
        for k in ("out_a", "out_v", "loss_a", "loss_v", "loss"):
            G.close(f"{tag}.s{s}.{k}", orc[k], ref[k])
            fx[f"{tag}.s{s}.{k}"] = ref[k].numpy()
        for k in ("head_grad_a", "head_grad_v"):
            G.close(f"{tag}.s{s}.{k}", orc[k], ref[k], rtol=1e-4, atol=1e-8)
        sd = model.module.state_dict()
        G.close(f"{tag}.s{s}.head.weight", st.head["weight"], sd["fusion_module.fc_out.weight"], rtol=1e-6, atol=1e-7)
        G.close(f"{tag}.s{s}.head.bias", st.head["bias"], sd["fusion_module.fc_out.bias"], rtol=1e-6, atol=1e-7)
        G.close(f"{tag}.s{s}.Pl", st.Pl, gs.Pl.detach(), rtol=1e-4, atol=1e-8)
        for k, vv in G.pl_digest(gs.Pl).items():
            if k != "rowsum":
                fx[f"{tag}.s{s}.Pl.{k}"] = np.asarray(vv)
    fc = model.module.fusion_module.fc_out
    mw, mb = opt.state[fc.weight]["momentum_buffer"], opt.state[fc.bias]["momentum_buffer"]
    G.close(f"{tag}.momentum.weight", st.mom["weight"], mw, rtol=1e-6, atol=1e-8)
    G.close(f"{tag}.momentum.bias", st.mom["bias"], mb, rtol=1e-6, atol=1e-8)
    W = fc.weight.detach()
    fx[f"{tag}.head.bias"] = fc.bias.detach().numpy().copy()
    fx[f"{tag}.momentum.bias"] = mb.numpy().copy()
    if gs_mode == "as_intended":
        fx[f"{tag}.head.weight"] = W.numpy().copy()
        fx[f"{tag}.momentum.weight"] = mw.numpy().copy()
    else:
        fx[f"{tag}.head.weight.col4"] = W[:, ::4].numpy().copy()
        fx[f"{tag}.momentum.weight.col4"] = mw[:, ::4].numpy().copy()
        fx[f"{tag}.head.weight.abssum"] = np.float64(W.double().abs().sum().item())
        fx[f"{tag}.momentum.weight.abssum"] = np.float64(mw.double().abs().sum().item())


if __name__ == "__main__":
    torch.set_num_threads(8)
    fx = {"meta": np.array([B, D, C, STEPS, SEED, LDL], dtype=np.int64)}
    run_mode(fx, "intended", "as_intended")
    run_mode(fx, "published", "as_published")
    path = os.path.join(HERE, "clip_small.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(f"  wrote {path} ({size / 1024:.1f} KiB)")
    assert size <= 700 * 1024, size
