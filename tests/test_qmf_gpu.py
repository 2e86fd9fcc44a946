"""GPU: the QMF joint step (--modulation QMF; main.py:170-268, 544-586) on the HIP kernels.

  * the head kernels through the C ABI against the reference's outputs (tests/golden/qmf_small.npz) and the fp64 test model, both
    loss forms, three steps with the History carried on the device; bitwise-equal reruns; index guards; duplicate indices;
  * QMFTrainer against the reference AVClassifier step case (conv_math f32 and split), overlap on / off, fc_out untouched;
  * the restated reference loop on the protocol objects equals QMFTrainer; QMFEvaluator counters;
  * one depth-1 M3AEClassifier and Modal3Classifier step (M = 3, the (0, 1) loss form) against the test model.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import qmf_model as Q  # noqa: E402
from oracle import mla_oracle as O  # noqa: E402
from util import assert_close, assert_close_robust  # noqa: E402

REL = 2e-5          # the project's per-kernel tolerance, relative to each tensor's largest element


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "qmf_small.npz"))


def rel_close(got, want, rel=REL, name=""):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    err, bound = (got - want).abs().max().item(), rel * want.abs().max().item()
    print(f"{name}: max|d| {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{name}: max|d|={err:.3e} > {bound:.3e}"


def _ops():
    from mla_hip import torch_ops  # noqa: F401
    return torch.ops.mla_hip


def _head_call(xs, Ws, bs, label, idx, corr, conf, form):
    w_cml, w_crl = Q.FORMS[form]
    return _ops().qmf_head_fwd_bwd(xs, Ws, bs, label, idx, corr, conf, w_cml, w_crl, 1.0 / xs[0].shape[0])


# ---- kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(Q.FORMS))
@pytest.mark.parametrize("shape", Q.HEAD_CASES, ids=lambda s: "_".join(map(str, s)))
def test_head_kernels_vs_reference_fixture(fx, shape, form):
    M, B, D, C, n_data = shape
    tag = Q.case_tag(shape, form)
    seed = int(fx[tag + ".seed"])
    corr = torch.zeros((M, n_data), dtype=torch.float64, device="cuda")
    conf_h = torch.zeros_like(corr)
    hists = [Q.History(n_data) for _ in range(M)]
    Ws_c, bs_c = Q.head_inputs(O, seed, M, B, D, C)[1:]
    Ws, bs = [w.cuda() for w in Ws_c], [b.cuda() for b in bs_c]
    for s in range(3):
        p = f"{tag}.s{s}."
        xs_c = Q.head_inputs(O, seed + s, M, B, D, C)[0]
        xs = [x.cuda() for x in xs_c]
        label, idx = torch.from_numpy(fx[p + "label"]).cuda(), torch.from_numpy(fx[p + "idx"]).cuda()
        before = (corr.clone(), conf_h.clone())
        got = _head_call(xs, Ws, bs, label, idx, corr, conf_h, form)
        torch.cuda.synchronize()
        z, out, conf, ell, target, margin, losses, dWs, dbs, dxs = got
        # the reference's outputs
        assert np.array_equal(target.cpu().numpy(), fx[p + "target"]), p + "target"
        for k, t in (("z", z), ("out", out), ("conf", conf), ("ell", ell), ("margin", margin), ("loss", losses[0]),
                     ("ce", losses[1:1 + M]), ("rank", losses[1 + M:1 + 2 * M]), ("cml", losses[1 + 2 * M]),
                     ("dW", torch.stack(dWs)), ("db", torch.stack(dbs)), ("dX", torch.stack(dxs))):
            Q.fixture_close(fx, p + k, t, REL)
        nz = fx[p + "hist_idx"]
        cc = corr.cpu().numpy()
        assert set(np.nonzero(cc.any(axis=0))[0].tolist()) == set(nz.tolist())
        Q.fixture_close(fx, p + "hist_correctness", cc[:, nz], REL)
        Q.fixture_close(fx, p + "hist_confidence", conf_h.cpu().numpy()[:, nz], REL)
        # the whole of every tensor against the fp64 model (the fixture samples the large ones)
        r = Q.qmf_step(xs_c, Ws_c, bs_c, fx[p + "label"], fx[p + "idx"], hists, *Q.FORMS[form])
        assert torch.equal(target.cpu().double(), r["target"])
        for k, t in (("dW", dWs), ("db", dbs), ("dX", dxs)):
            rel_close(torch.stack(t), torch.stack(r[k]), name=p + k + " vs model")
        rel_close(corr, np.stack([h.correctness for h in hists]), name=p + "history vs model")
        # two runs from the same state are bitwise equal
        corr2, conf2 = before
        again = _head_call(xs, Ws, bs, label, idx, corr2, conf2, form)
        torch.cuda.synchronize()
        for a, b in zip(got[:7], again[:7]):
            assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num())
        for la, lb in zip(got[7:], again[7:]):
            for a, b in zip(la, lb):
                assert torch.equal(a, b)
        assert torch.equal(corr, corr2) and torch.equal(conf_h, conf2)
        # forward-only variant: one launch, the same logits
        fz, fout, fconf = _ops().qmf_head_fwd(xs, Ws, bs)
        assert torch.equal(fz, z) and torch.equal(fout, out) and torch.equal(fconf, conf)


def test_out_of_range_index_gives_nan_for_that_row_only():
    """An input guard on a valid launch: the sample with a bad index gets NaN losses and writes nothing."""
    M, B, D, C, n_data = 2, 6, 512, 6, 9
    xs_c, Ws_c, bs_c = Q.head_inputs(O, 5, M, B, D, C)
    xs, Ws, bs = [x.cuda() for x in xs_c], [w.cuda() for w in Ws_c], [b.cuda() for b in bs_c]
    label = O.portable_labels(5, B, C).cuda()
    for bad in (n_data, -1, 2 ** 40):
        idx = torch.tensor([3, 1, bad, 7, 0, 5], device="cuda")
        corr = torch.full((M, n_data), 0.25, dtype=torch.float64, device="cuda")
        conf_h = torch.full_like(corr, 0.5)
        z, out, conf, ell, target, margin, losses, dWs, dbs, dxs = _head_call(xs, Ws, bs, label, idx, corr, conf_h, "av")
        torch.cuda.synchronize()
        nan = torch.isnan(ell).cpu()
        assert nan[:, 2].all() and not nan[:, [0, 1, 3, 4, 5]].any()
        assert torch.isnan(losses[0]) and torch.isnan(losses[1:1 + M]).all()
        assert torch.isfinite(z).all() and torch.isfinite(out).all()
        assert all(torch.isfinite(t).all() for t in dWs + dbs + dxs) and all(float(t[2].abs().max()) == 0.0 for t in dxs)
        good = [3, 1, 7, 0, 5]
        rows = [0, 1, 3, 4, 5]
        cc, cf = corr.cpu(), conf_h.cpu()
        untouched = [k for k in range(n_data) if k not in good]
        assert (cc[:, untouched] == 0.25).all() and (cf[:, untouched] == 0.5).all()
        assert torch.equal(cc[:, good], 0.25 + ell.cpu()[:, rows].double())
        assert torch.equal(cf[:, good], conf.cpu()[:, rows].double())


def test_duplicate_index_inside_a_batch_matches_the_model():
    M, B, D, C, n_data = 2, 7, 512, 6, 6
    xs_c, Ws_c, bs_c = Q.head_inputs(O, 9, M, B, D, C)
    idx = np.array([4, 1, 4, 2, 1, 4, 0])
    label = O.portable_labels(9, B, C)
    hists = [Q.History(n_data) for _ in range(M)]
    corr = torch.zeros((M, n_data), dtype=torch.float64, device="cuda")
    conf_h = torch.zeros_like(corr)
    for _ in range(2):
        r = Q.qmf_step(xs_c, Ws_c, bs_c, label, idx, hists, 1.0, 0.1)
        got = _head_call([x.cuda() for x in xs_c], [w.cuda() for w in Ws_c], [b.cuda() for b in bs_c], label.cuda(),
                         torch.from_numpy(idx).cuda(), corr, conf_h, "av")
        torch.cuda.synchronize()
        rel_close(corr, np.stack([h.correctness for h in hists]), name="correctness")
        rel_close(conf_h, np.stack([h.confidence for h in hists]), name="confidence")
        assert torch.equal(got[4].cpu().double(), r["target"])
        rel_close(got[6][0], r["loss"], name="loss")
    ell = got[3].cpu().double()
    assert float(corr[0, 4]) == 2 * float(ell[0, 5]) and float(corr[0, 1]) == 2 * float(ell[0, 4])       # the last occurrence alone


# ---- QMFTrainer vs the reference AVClassifier step case ---------------------------------------------------------------------
class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
    lorb, clip, modal3 = "base", False, False


def _av_state(seed):
    sd = {f"module.audio_net.{k}": v for k, v in O.make_resnet18_params("audio", seed).items()}
    sd.update({f"module.visual_net.{k}": v for k, v in O.make_resnet18_params("visual", seed + 1).items()})
    sd.update({f"module.fusion_module.fc_out.{k}": v for k, v in O.make_head_params(1024, 6, seed + 2).items()})
    sd.update({f"module.audio_fc.{k}": v for k, v in O.make_head_params(512, 6, seed + 3).items()})
    sd.update({f"module.visual_fc.{k}": v for k, v in O.make_head_params(512, 6, seed + 4).items()})
    return sd


def _av_inputs(seed, s, B, spec_hw, T, img_hw):
    spec = O.portable_normal(seed + 100 + s, (B,) + tuple(spec_hw), stream=1, mean=-5.081, std=4.4849)
    image = O.portable_normal(seed + 100 + s, (B, 3, T) + tuple(img_hw), stream=2)
    return spec.cuda(), image.cuda(), O.portable_labels(seed + 100 + s, B, 6).cuda()


def _build_av(seed, n_data, conv_math="f32"):
    from mla_hip import AVClassifier, QMFTrainer, attach_qmf_heads
    model = AVClassifier(AVArgs(), seed=0, conv_math=conv_math)
    attach_qmf_heads(model, seed=0)
    model.load_state_dict(_av_state(seed))
    return model, QMFTrainer(model, n_data, lr=1e-3, momentum=0.9, weight_decay=1e-4)


@pytest.mark.parametrize("conv_math", ["f32", "split"])
def test_qmf_step_vs_reference_golden(fx, conv_math):
    B, sh, sw, T, ih, iw, steps, seed, n_data = [int(v) for v in fx["av.meta"]]
    model, tr = _build_av(seed, n_data, conv_math)
    fc = model.fusion_module.fc_out
    assert torch.equal(fc.weight.detach().cpu(), torch.from_numpy(fx["av.fc_out.weight.before"]))
    for s in range(steps):
        spec, image, label = _av_inputs(seed, s, B, (sh, sw), T, (ih, iw))
        idx = torch.from_numpy(fx[f"av.s{s}.idx"]).cuda()                  # (B, 1), as the loader yields it
        losses = tr.train_step(spec, image, label, idx, s)
        torch.cuda.synchronize()
        p = f"av.s{s}."
        tol = 2e-4 if s == 0 else 1e-3          # step 1 is free-running (see test_step_gpu.py)
        for k in ("a", "v", "out", "conf"):
            assert_close(tr.last[k], fx[p + k], atol=tol, name=p + k)
        assert_close(tr.last["out_m"][0], fx[p + "out_a"], atol=tol, name=p + "out_a")
        assert_close(tr.last["out_m"][1], fx[p + "out_v"], atol=tol, name=p + "out_v")
        assert np.array_equal(tr.last["target"].cpu().numpy(), fx[p + "target"]), p + "target"
        assert_close(tr.last["rank"], fx[p + "rank"], atol=tol, name=p + "rank")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), fx[p + k], atol=tol, name=p + k)
        for nm in ("audio_fc", "visual_fc"):
            head = getattr(model, nm)
            assert_close(head.weight_grad, fx[p + f"{nm}.weight.grad"], atol=tol, name=p + nm + " grad")
            assert_close(head.bias_grad, fx[p + f"{nm}.bias.grad"], atol=tol, name=p + nm + " bias grad")
        sd = model.state_dict()
        for nm in ("audio_fc", "visual_fc"):
            assert_close(sd[f"{nm}.weight"], fx[p + f"{nm}.weight"], atol=tol, name=p + nm + " weight")
            assert_close(sd[f"{nm}.bias"], fx[p + f"{nm}.bias"], atol=tol, name=p + nm + " bias")
        assert_close(tr.history.correctness, fx[p + "hist_correctness"], atol=tol, name=p + "history correctness")
        assert_close(tr.history.confidence, fx[p + "hist_confidence"], atol=tol, name=p + "history confidence")
        enc_g = {"audio_net": model.audio_net.grads_as_reference(), "visual_net": model.visual_net.grads_as_reference()}
        for enc in ("audio_net", "visual_net"):
            assert_close(sd[f"{enc}.bn1.running_mean"], fx[p + f"{enc}.bn1.running_mean"], atol=1e-5, rtol=1e-5, name="running_mean")
            assert_close(sd[f"{enc}.bn1.running_var"], fx[p + f"{enc}.bn1.running_var"], atol=1e-5, rtol=1e-5, name="running_var")
            assert_close_robust(sd[f"{enc}.conv1.weight"], fx[p + f"{enc}.conv1.weight"], rel_l2=2e-3, elem_tol=2e-3, frac=0.9,
                                name=f"{p}{enc} conv1.weight")
            w = sd[f"{enc}.layer4.1.conv2.weight"]
            assert_close(w.flatten()[:64], fx[p + f"{enc}.layer4.1.conv2.weight.head"], atol=2e-6, name="layer4 weight slice")
            assert abs(w.double().sum().item() - float(fx[p + f"{enc}.layer4.1.conv2.weight.sum"])) < 1e-3
            pre = p + f"grad.{enc}."
            for key in [k for k in fx.files if k.startswith(pre) and k.endswith(".abssum")]:
                g_ = enc_g[enc][key[len(pre):-len(".abssum")]]
                got, want = g_.double().abs().sum().item(), float(fx[key])
                assert abs(got - want) <= 5e-3 * want + 1e-9, f"{key}: {got} vs {want}"
                assert_close_robust(g_.flatten()[:64], fx[key[:-len(".abssum")] + ".head"], rel_l2=5e-2 if s == 0 else 1e-1,
                                    elem_tol=1.0, frac=0.0, name=key[:-len(".abssum")] + ".head")
    # fusion_module.fc_out is constructed and never used: no gradient, so SGD (weight decay included) leaves it bit for bit
    assert torch.equal(fc.weight.detach().cpu(), torch.from_numpy(fx["av.fc_out.weight.before"]))
    assert torch.equal(fc.bias.detach().cpu(), torch.from_numpy(fx["av.fc_out.bias.before"]))


def test_overlap_off_is_bitwise_equal_to_overlap_on(fx):
    B, sh, sw, T, ih, iw, steps, seed, n_data = [int(v) for v in fx["av.meta"]]
    res = []
    for overlap in (True, False):
        model, tr = _build_av(seed, n_data)
        tr.set_overlap(overlap)
        for s in range(steps):
            spec, image, label = _av_inputs(seed, s, B, (sh, sw), T, (ih, iw))
            tr.train_step(spec, image, label, torch.from_numpy(fx[f"av.s{s}.idx"]).cuda(), s)
        tr.join()
        torch.cuda.synchronize()
        res.append((model.state_dict(), tr.history.correctness.clone(), tr.losses["loss"].clone()))
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_reference_loop_on_protocol_objects_equals_qmf_trainer(fx):
    """main.py:164, 240-268, 304-310, 412 restated (torch ops on the device, the numpy History of tests/qmf_model.py) on an attached
    model with FusedSGD, against QMFTrainer from the same state: losses and head gradients to 2e-5 relative on step 0."""
    import mla_hip
    B, sh, sw, T, ih, iw, _steps, seed, n_data = [int(v) for v in fx["av.meta"]]
    ref = mla_hip.AVClassifier(AVArgs(), seed=0, conv_math="f32")
    mla_hip.attach_qmf_heads(ref, seed=0)
    ref.load_state_dict(_av_state(seed))
    model = torch.nn.DataParallel(ref, device_ids=[0])
    optimizer = mla_hip.FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    fused, tr = _build_av(seed, n_data)
    spec, image, label = _av_inputs(seed, 0, B, (sh, sw), T, (ih, iw))
    idx = torch.from_numpy(fx["av.s0.idx"])
    criterion = nn.CrossEntropyLoss()
    txt_history, img_history = Q.History(n_data), Q.History(n_data)
    model.train()
    optimizer.zero_grad()
    out_a, out_v = model(spec.unsqueeze(1).float(), image.float())
    txt_energy = torch.log(torch.sum(torch.exp(out_a), dim=1))
    img_energy = torch.log(torch.sum(torch.exp(out_v), dim=1))
    txt_conf = torch.reshape(txt_energy / 10, (-1, 1))
    img_conf = torch.reshape(img_energy / 10, (-1, 1))
    out = (out_a * txt_conf.detach() + out_v * img_conf.detach())
    clf_loss = nn.CrossEntropyLoss()(out_a, label) + nn.CrossEntropyLoss()(out_v, label)
    txt_loss = nn.CrossEntropyLoss(reduction='none')(out_a, label).detach()
    img_loss = nn.CrossEntropyLoss(reduction='none')(out_v, label).detach()
    ranks = []
    for h, l, c in ((txt_history, txt_loss, txt_conf), (img_history, img_loss, img_conf)):
        h.update(idx.numpy(), l.cpu().numpy(), c.detach().squeeze(1).cpu().numpy())
        t, mg = h.target_margin(idx.numpy())
        ranks.append(Q.rank_loss(c.squeeze(1), t, np.float32(mg)))
    cml_loss = nn.CrossEntropyLoss()(out, label)
    loss = cml_loss + clf_loss + 0.1 * (ranks[0] + ranks[1])
    loss_a, loss_v = criterion(out_a, label), criterion(out_v, label)
    loss.backward()
    head_grads = [ref.audio_fc.weight.grad.clone(), ref.visual_fc.weight.grad.clone(), ref.audio_fc.bias.grad.clone(),
                  ref.visual_fc.bias.grad.clone()]
    assert ref.fusion_module.fc_out.weight.grad is None
    optimizer.step()
    losses = tr.train_step(spec, image, label, idx.cuda(), 0)
    torch.cuda.synchronize()
    rel_close(tr.last["out"], out.detach(), name="out")
    for k, want in (("loss", loss), ("loss_a", loss_a), ("loss_v", loss_v)):
        rel_close(losses[k].reshape(()), want.detach().reshape(()), name=k)
    for got, want, name in zip([fused.audio_fc.weight_grad, fused.visual_fc.weight_grad, fused.audio_fc.bias_grad,
                                fused.visual_fc.bias_grad], head_grads, ("audio_fc dW", "visual_fc dW", "audio_fc db", "visual_fc db")):
        rel_close(got, want, name=name)
    sd_r, sd_f = ref.state_dict(), fused.state_dict()
    for k in ("audio_fc.weight", "visual_fc.weight", "fusion_module.fc_out.weight"):
        assert_close(sd_f[k], sd_r[k], atol=1e-6, name=k)
    rel_close(tr.history.correctness, np.stack([txt_history.correctness, img_history.correctness]), name="history")


def test_qmf_evaluator_counts():
    from mla_hip import AVClassifier, QMFEvaluator, attach_qmf_heads
    B, C = 32, 6
    model = AVClassifier(AVArgs(), seed=0)
    heads = attach_qmf_heads(model, seed=4)
    with torch.no_grad():
        for h in heads:
            h.weight.mul_(3.0)
    feats = [O.portable_normal(3, (B, 512), stream=60 + m) for m in range(2)]
    label = O.portable_labels(3, B, C)
    z = [feats[m].double() @ heads[m].weight.detach().cpu().double().T + heads[m].bias.detach().cpu().double() for m in range(2)]
    out = sum(torch.logsumexp(z[m], 1, keepdim=True) / 10 * z[m] for m in range(2))
    preds = [o.argmax(1) for o in (out, z[0], z[1])]
    assert (preds[0] != preds[1]).any() and (preds[0] != preds[2]).any()          # the fused arg-max is no copy of a head's
    for o in (out, z[0], z[1]):                                                  # and no arg-max hangs on an fp32 rounding
        top = o.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) > 1e-4
    dev = [f.cuda() for f in feats]
    model.forward_raw = lambda *a: dev                                            # the encoders are not what is counted here
    ev = QMFEvaluator(model)
    got_out, got_z = ev.update(None, None, label.cuda())
    torch.cuda.synchronize()
    rel_close(got_out, out, name="eval out")
    rel_close(got_z, torch.stack(z), name="eval out_m")
    want = tuple(float((p == label).sum()) / B for p in preds)
    assert ev.result() == want, (ev.result(), want)
    counts = ev.counts.view(5, C).cpu()
    for c in range(C):
        assert int(counts[0, c]) == int((label == c).sum())
        for row, p in ((1, preds[0]), (3, preds[1]), (4, preds[2])):
            assert int(counts[row, c]) == int(((p == label) & (label == c)).sum())


# ---- M3AE / Modal3: M = 3 and the (0, 1) loss form end to end ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["m3ae", "modal3"])
def test_transformer_qmf_step_vs_model(which):
    import mla_hip
    B, vocab, n_data = 2, 64, 5

    class A:
        fusion_method, gs_flag, modulation = "concat", False, "Normal"
    A.dataset = "MVSA" if which == "m3ae" else "IEMOCAP"
    cls = mla_hip.M3AEClassifier if which == "m3ae" else mla_hip.Modal3Classifier
    model = cls(A(), depth=1, text_vocab_size=vocab, seed=0)
    tr = mla_hip.QMFTrainer(model, n_data, seed=11)
    assert (tr.w_cml, tr.w_crl) == (0.0, 1.0) and tr.M == (2 if which == "m3ae" else 3)
    token = torch.from_numpy(np.minimum((O.portable_uniform(5, B * 256, 7) * vocab).astype(np.int64), vocab - 1)).view(B, 1, 256)
    pm = torch.zeros(B, 1, 256)
    for b in range(B):
        pm[b, 0, 30 + 41 * b:] = 1.0
    image = O.portable_normal(5, (B, 3, 256, 256), stream=3)
    spec = O.portable_normal(5, (B, 1024, 128), stream=4, mean=-5.081, std=4.4849)
    inputs = [token, pm, image] + ([spec] if which == "modal3" else [])
    label = O.portable_labels(5, B, tr.heads[0].out_features)
    hists = [Q.History(n_data) for _ in range(tr.M)]
    fc_before = model.fusion_module.fc_out.flat.clone()
    tags = [t for t, _g, _e in model.mla_encoders()]
    for s, idx in enumerate(([3, 1], [1, 4])):
        Ws = [h.weight.detach().cpu().clone() for h in tr.heads]
        bs = [h.bias.detach().cpu().clone() for h in tr.heads]
        losses = tr.train_step(*[x.cuda() for x in inputs], label.cuda(), torch.tensor(idx).cuda(), s)
        tr.join()
        torch.cuda.synchronize()
        r = Q.qmf_step([tr.last[t].cpu() for t in tags], Ws, bs, label, idx, hists, 0.0, 1.0)      # the HIP path's own features
        assert torch.equal(tr.last["target"].cpu().double(), r["target"])
        rel_close(tr.last["out"], r["out"], name=f"{which} s{s} out")
        rel_close(tr.last["out_m"], r["z"], name=f"{which} s{s} out_m")
        rel_close(losses["loss"].reshape(()), r["loss"], name=f"{which} s{s} loss")
        for k, t in enumerate(tags):
            rel_close(losses["loss_" + t].reshape(()), r["ce"][k], name=f"{which} s{s} loss_{t}")
            rel_close(tr.heads[k].weight_grad, r["dW"][k], name=f"{which} s{s} dW_{t}")
            rel_close(tr.heads[k].bias_grad, r["db"][k], name=f"{which} s{s} db_{t}")
        rel_close(tr.history.correctness, np.stack([h.correctness for h in hists]), name=f"{which} s{s} history")
    assert torch.equal(model.fusion_module.fc_out.flat, fc_before)
