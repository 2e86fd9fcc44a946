"""Fixture generator for the QMF joint step (--modulation QMF; main.py:170-268, 108-125; utils/utils.py:44-95).

Runs only where the reference tree is available (read-only).  It drives the reference's unmodified `AVClassifier` (modulation
"QMF", gs_flag false: audio_fc / visual_fc beside the unused ConcatFusion, basic_model.py:31-34, 45-47, 67-71) and
`utils.utils.History` (whose get_target_margin calls `.cuda()`: torch.Tensor.cuda is stubbed to the identity for the run), with
nn.CrossEntropyLoss, nn.MarginRankingLoss and torch.optim.SGD(lr 1e-3, momentum 0.9, weight decay 1e-4).  Only the inline loop lines
(main.py:239-268, 304-310, 416) and rank_loss (main.py:108-125) are restated around them.  Writes qmf_small.npz (data only):

  head-level cases `head.<M>_<B>_<D>_<C>_<n>.<form>` (form `av`: loss = cml + clf + 0.1 crl, main.py:265-268; `m3ae`: clf + crl,
    main.py:203, 229) on portable-PRNG features (tests/qmf_model.py: head_inputs), nn.Linear heads, three consecutive steps on
    overlapping index sets with the History carried: labels, idx, z, out, conf, ell, target, margin, cml / ce / rank / loss, head
    gradients, dX and the History after each step (its non-zero entries).  Tensors above 2048 elements are recorded as up to
    256 sampled positions per modality plus the fp64 sum of absolute values.  The seed of a case is searched so that the reference alone
    meets the conditions tests/test_qmf_cpu.py asserts (every target value occurs, the hinge is active and inactive, no margin or
    hinge argument within 1e-4 of a decision);
  `av`: two steps of the reference AVClassifier at the joint fixture's shapes: what joint_small.npz records, plus the audio_fc /
    visual_fc gradients and post-step values, fusion_module.fc_out (the steps leave it bit for bit unchanged), the History, the state_dict keys and shapes.

    python tests/golden/make_golden_qmf.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_joint as J  # noqa: E402  (imports the reference modules through make_golden.py)
from make_golden_joint import G, O  # noqa: E402
from utils.utils import History  # noqa: E402  (reference)
import qmf_model as Q  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self            # History.get_target_margin: `.float().cuda()` (utils/utils.py:90, 93)

HEAD_CASES = [(2, 5, 512, 6, 11), (3, 4, 768, 4, 9), (2, 3, 768, 101, 7), (2, 1, 512, 6, 3), (2, 64, 512, 6, 70001)]
FORMS = {"av": (1.0, 0.1), "m3ae": (0.0, 1.0)}
BIG = 2048


def rank_loss(confidence, idx, history, rec):
    """main.py:108-125 (the `rec` lines are the only additions)."""
    # make input pair
    rank_input1 = confidence
    rank_input2 = torch.roll(confidence, -1)
    idx2 = torch.roll(idx, -1)

    # calc target, margin
    if idx2.numel() == 1:       # B = 1: numpy takes a one-element tensor for a scalar index and History's `[:n_pair]` then raises;
        idx2 = idx2.numpy()     # handed over as an array, History computes the pair of the sample with itself
    rank_target, rank_margin = history.get_target_margin(idx, idx2)
    rec["target"].append(rank_target.reshape(-1).clone())
    rec["margin"].append(rank_margin.reshape(-1).clone())
    rank_target_nonzero = rank_target.clone()
    rank_target_nonzero[rank_target_nonzero == 0] = 1
    rank_input2 = rank_input2 + (rank_margin / rank_target_nonzero).reshape((-1, 1))
    rec["hinge_arg"].append((rank_target.reshape(-1, 1) * (rank_input1 - rank_input2)).detach().reshape(-1).clone())

    # ranking loss
    ranking_loss = nn.MarginRankingLoss(margin=0.0)(rank_input1,
                                                    rank_input2,
                                                    -rank_target.reshape(-1, 1))

    return ranking_loss


def qmf_losses(outs, label, idx, hists, form, rec):
    """main.py:242-268 (form "av") / :173-203, 206-229 (form "m3ae") for M modalities, restated around the reference's History."""
    confs = []
    for o in outs:
        energy = torch.log(torch.sum(torch.exp(o), dim=1))
        confs.append(torch.reshape(energy / 10, (-1, 1)))
    out = sum(o * c.detach() for o, c in zip(outs, confs))
    clfs = [nn.CrossEntropyLoss()(o, label) for o in outs]
    clf_loss = sum(clfs)
    ells = [nn.CrossEntropyLoss(reduction='none')(o, label).detach() for o in outs]
    for h, l, c in zip(hists, ells, confs):
        h.correctness_update(idx, l, c.squeeze(1))
    ranks = [rank_loss(c, idx, h, rec) for c, h in zip(confs, hists)]
    crl_loss = sum(ranks)
    cml_loss = nn.CrossEntropyLoss()(out, label)
    if form == "av":
        loss = cml_loss + clf_loss + 0.1 * crl_loss
    else:
        loss = torch.mean(clf_loss + crl_loss)
    rec.update(out=out, conf=torch.stack([c.detach().reshape(-1) for c in confs]), ell=torch.stack(ells),
               ce=torch.stack([c.detach() for c in clfs]), rank=torch.stack([r.detach() for r in ranks]), cml=cml_loss.detach(),
               loss=loss.detach())
    return loss


def put(fx, key, t):
    t = np.asarray(t.detach() if isinstance(t, torch.Tensor) else t)
    if t.size <= BIG:
        fx[key] = t
        return
    flat = t.reshape(t.shape[0], -1)
    pos = np.unique(np.minimum((O.portable_uniform(11, 256, 55) * flat.shape[1]).astype(np.int64), flat.shape[1] - 1))
    fx[key + ".pos"] = pos
    fx[key + ".sub"] = flat[:, pos].copy()
    fx[key + ".abssum"] = np.float64(np.abs(flat.astype(np.float64)).sum())


def case_indices(seed, s, B, n_data, prev):
    """Overlapping index sets: half of a step's indices come from the step before; from step 1 on one adjacent and (B >= 4) one
    distant duplicate inside the batch."""
    idx = np.minimum((O.portable_uniform(seed + 7 * s, B, 77) * n_data).astype(np.int64), n_data - 1)
    if prev is not None:
        idx[:B // 2] = np.roll(prev, 1)[:B // 2]
        if B >= 2:
            idx[1] = idx[0]
        if B >= 4:
            idx[B - 1] = idx[2]
    return idx


def run_head_case(shape, form, seed):
    M, B, D, C, n_data = shape
    hists = [History(n_data) for _ in range(M)]
    steps, prev = [], None
    for s in range(3):
        xs, Ws, bs = Q.head_inputs(O, seed + s, M, B, D, C)
        Ws, bs = Q.head_inputs(O, seed, M, B, D, C)[1:]                       # the heads stay; the features change per step
        heads = [nn.Linear(D, C) for _ in range(M)]
        for h, W, b in zip(heads, Ws, bs):
            h.load_state_dict({"weight": W, "bias": b})
        xs = [x.clone().requires_grad_(True) for x in xs]
        label = O.portable_labels(seed + s, B, C)
        idx = case_indices(seed, s, B, n_data, prev)
        prev = idx
        rec = {"target": [], "margin": [], "hinge_arg": []}
        outs = [h(x) for h, x in zip(heads, xs)]
        loss = qmf_losses(outs, label, torch.from_numpy(idx).reshape(-1, 1), hists, form, rec)
        loss.backward()
        rec.update(z=torch.stack([o.detach() for o in outs]), label=label, idx=idx,
                   dW=torch.stack([h.weight.grad for h in heads]), db=torch.stack([h.bias.grad for h in heads]),
                   dX=torch.stack([x.grad for x in xs]))
        for k in ("target", "margin", "hinge_arg"):
            rec[k] = torch.stack(rec[k])
        nz = np.unique(np.concatenate([np.nonzero(h.correctness)[0] for h in hists]))
        rec["hist_idx"] = nz
        rec["hist_correctness"] = np.stack([h.correctness[nz] for h in hists])
        rec["hist_confidence"] = np.stack([h.confidence[nz] for h in hists])
        steps.append(rec)
    return steps


def conditions(steps, B):
    """What tests/test_qmf_cpu.py asserts on the fixture (the B = 1 case pairs a sample with itself: its targets are all 0)."""
    t = torch.cat([r["target"].reshape(-1) for r in steps])
    mg = torch.cat([r["margin"].reshape(-1) for r in steps])
    ha = torch.cat([r["hinge_arg"].reshape(-1) for r in steps])
    if not (torch.isfinite(mg).all() and torch.isfinite(ha).all()):
        return False
    ok = bool((mg[mg != 0] > 1e-4).all()) and bool((ha[t != 0].abs() > 1e-4).all())
    if B > 1:
        ok = ok and all(bool((t == v).any()) for v in (-1.0, 0.0, 1.0)) and bool((ha > 0).any()) and bool((ha[t != 0] < 0).any())
    return ok


def run_head_cases(fx):
    for shape in HEAD_CASES:
        for form in FORMS:
            for seed in range(300, 400):
                steps = run_head_case(shape, form, seed)
                if conditions(steps, shape[1]):
                    break
            else:
                raise RuntimeError(f"no seed meets the conditions for {shape} {form}")
            tag = "head." + "_".join(str(v) for v in shape) + "." + form
            print(f"== {tag}: seed {seed}")
            fx[tag + ".seed"] = np.int64(seed)
            for s, rec in enumerate(steps):
                for k in ("label", "idx", "z", "out", "conf", "ell", "target", "margin", "hinge_arg", "ce", "rank", "cml", "loss",
                          "dW", "db", "dX", "hist_idx", "hist_correctness", "hist_confidence"):
                    put(fx, f"{tag}.s{s}.{k}", rec[k])


class _QMFArgs(G._Args):
    gs_flag = False
    modulation = "QMF"


AV_IDX = [[2, 5, 5, 8], [5, 2, 9, 2]]
AV_NDATA = 10


def run_av_case(fx, B=4, spec_hw=(128, 64), T=2, img_hw=(96, 96), steps=2, seed=7):
    print(f"== qmf av case: B={B} spec={spec_hw} T={T} img={img_hw} steps={steps}")
    torch.manual_seed(0)
    model = G.AVClassifier(_QMFArgs())
    model.audio_net.load_state_dict(O.make_resnet18_params("audio", seed))
    model.visual_net.load_state_dict(O.make_resnet18_params("visual", seed + 1))
    model.fusion_module.fc_out.load_state_dict(O.make_head_params(1024, 6, seed + 2))
    model.audio_fc.load_state_dict(O.make_head_params(512, 6, seed + 3))
    model.visual_fc.load_state_dict(O.make_head_params(512, 6, seed + 4))
    model = torch.nn.DataParallel(model)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)       # main.py:749
    criterion = nn.CrossEntropyLoss()
    txt_history, img_history = History(AV_NDATA), History(AV_NDATA)
    feats = {}
    hooks = [model.module.audio_fc.register_forward_hook(lambda m, i, o: feats.__setitem__("a", i[0].detach().clone())),
             model.module.visual_fc.register_forward_hook(lambda m, i, o: feats.__setitem__("v", i[0].detach().clone()))]
    fc = model.module.fusion_module.fc_out
    fx["av.fc_out.weight.before"] = fc.weight.detach().numpy().copy()
    fx["av.fc_out.bias.before"] = fc.bias.detach().numpy().copy()
    for s in range(steps):
        spec = O.portable_normal(seed + 100 + s, (B,) + spec_hw, stream=1, mean=-5.081, std=4.4849)
        image = O.portable_normal(seed + 100 + s, (B, 3, T) + img_hw, stream=2)
        label = O.portable_labels(seed + 100 + s, B, 6)
        idx = torch.tensor(AV_IDX[s], dtype=torch.int64).reshape(-1, 1)
        rec = {"target": [], "margin": [], "hinge_arg": []}
        model.train()
        opt.zero_grad()                                                                        # main.py:164
        out_a, out_v = model(spec.unsqueeze(1).float(), image.float())                         # :240
        loss = qmf_losses([out_a, out_v], label, idx, [txt_history, img_history], "av", rec)   # :242-268
        loss_a = criterion(out_a, label)                                                       # :308
        loss_v = criterion(out_v, label)                                                       # :309
        loss.backward()                                                                        # :310
        p = f"av.s{s}."
        for k, t in (("a", feats["a"]), ("v", feats["v"]), ("out", rec["out"]), ("out_a", out_a), ("out_v", out_v), ("loss", loss),
                     ("loss_a", loss_a), ("loss_v", loss_v), ("conf", rec["conf"]), ("rank", rec["rank"]), ("cml", rec["cml"]),
                     ("target", torch.stack(rec["target"])), ("margin", torch.stack(rec["margin"])),
                     ("hinge_arg", torch.stack(rec["hinge_arg"]))):
            fx[p + k] = t.detach().numpy().copy()
        fx[p + "idx"] = idx.numpy().copy()
        grads = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None}
        assert fc.weight.grad is None and fc.bias.grad is None                                 # constructed, never used under QMF
        for nm in ("audio_fc", "visual_fc"):
            fx[p + f"{nm}.weight.grad"] = grads[f"module.{nm}.weight"].numpy()
            fx[p + f"{nm}.bias.grad"] = grads[f"module.{nm}.bias"].numpy()
        for enc in ("audio_net", "visual_net"):
            for k in J.KEEP:
                g = grads[f"module.{enc}.{k}"]
                fx[p + f"grad.{enc}.{k}.abssum"] = np.float64(g.double().abs().sum().item())
                fx[p + f"grad.{enc}.{k}.head"] = g.flatten()[:64].numpy().copy()
        opt.step()                                                                             # :416
        sd = model.module.state_dict()
        for nm in ("audio_fc", "visual_fc"):
            fx[p + f"{nm}.weight"] = sd[f"{nm}.weight"].numpy().copy()
            fx[p + f"{nm}.bias"] = sd[f"{nm}.bias"].numpy().copy()
        for enc in ("audio_net", "visual_net"):
            fx[p + f"{enc}.bn1.running_mean"] = sd[f"{enc}.bn1.running_mean"].numpy().copy()
            fx[p + f"{enc}.bn1.running_var"] = sd[f"{enc}.bn1.running_var"].numpy().copy()
            fx[p + f"{enc}.conv1.weight"] = sd[f"{enc}.conv1.weight"].numpy().copy()
            w = sd[f"{enc}.layer4.1.conv2.weight"]
            fx[p + f"{enc}.layer4.1.conv2.weight.sum"] = np.float64(w.double().sum().item())
            fx[p + f"{enc}.layer4.1.conv2.weight.head"] = w.flatten()[:64].numpy().copy()
        fx[p + "hist_correctness"] = np.stack([txt_history.correctness, img_history.correctness])
        fx[p + "hist_confidence"] = np.stack([txt_history.confidence, img_history.confidence])
        print(f"   step {s}: loss {float(loss):.5f} targets {fx[p + 'target'].tolist()} min |hinge arg| "
              f"{np.abs(fx[p + 'hinge_arg'][fx[p + 'target'] != 0]).min():.3e} margins {fx[p + 'margin'].tolist()}")
    for h in hooks:
        h.remove()
    assert np.array_equal(fx["av.fc_out.weight.before"], fc.weight.detach().numpy())          # SGD never touched it
    assert np.array_equal(fx["av.fc_out.bias.before"], fc.bias.detach().numpy())
    fx["av.meta"] = np.array([B, spec_hw[0], spec_hw[1], T, img_hw[0], img_hw[1], steps, seed, AV_NDATA], dtype=np.int64)
    sd = model.state_dict()
    fx["state_keys"] = np.array(list(sd.keys()))
    fx["state_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


if __name__ == "__main__":
    torch.set_num_threads(8)
    fx = {}
    run_head_cases(fx)
    run_av_case(fx)
    path = os.path.join(HERE, "qmf_small.npz")
    np.savez_compressed(path, **fx)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
