"""GPU: the joint concat-fusion step (gs_flag false; main.py:164-168, 273-311, 312-417) on the HIP kernels.

  * the concatenated-head kernels against an fp64 torch restatement (every variant, M 2 / 3, D 512 / 768, C 6 / 101,
    B 1 / 5 / 64), NaN on a bad label, bitwise-equal reruns;
  * the fused JointTrainer against the reference's outputs (tests/golden/joint_small.npz, make_golden_joint.py) for Normal
    and OGM, with the tolerances of tests/test_step_gpu.py;
  * the reference's own loop (main.py:164-168, 273-311, 312-417 verbatim: torch CrossEntropyLoss, DataParallel,
    named_parameters() modulation) on the protocol objects equals the fused JointTrainer, for AV, M3AE and Modal3;
  * the M3AE joint step against the reference's outputs (joint_small.npz, `m3ae` case);
  * OGM-GE reproducibility and noise scale; JointEvaluator counters.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from util import assert_close, assert_close_robust  # noqa: E402

TOL = 2e-4


# ---- kernels --------------------------------------------------------------------------------------------------------------
def _ref_head(xs, W, b, label):
    xs64 = [x.double().cpu() for x in xs]
    W64, b64 = W.double().cpu(), b.double().cpu()
    M, (B, D) = len(xs), xs[0].shape
    cat = torch.cat(xs64, dim=1)
    out = cat @ W64.T + b64
    out_m = torch.stack([xs64[m] @ W64[:, m * D:(m + 1) * D].T + b64 / M for m in range(M)])
    lab = label.cpu()
    lsm = torch.log_softmax(out, dim=1)
    loss = -lsm[torch.arange(B), lab].mean()
    loss_m = torch.stack([-torch.log_softmax(out_m[m], 1)[torch.arange(B), lab].mean() for m in range(M)])
    dl = (torch.softmax(out, 1) - torch.nn.functional.one_hot(lab, W.shape[0]).double()) / B
    return out, out_m, loss, loss_m, dl, dl.T @ cat, dl.sum(0), [dl @ W64[:, m * D:(m + 1) * D] for m in range(M)]


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("D", [512, 768])
@pytest.mark.parametrize("C", [6, 101])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_concat_head_kernels_vs_fp64(M, D, C, B):
    from mla_hip import torch_ops  # noqa: F401
    T = torch.ops.mla_hip
    g = torch.Generator().manual_seed(1000 * M + D + 7 * C + B)
    xs = [torch.randn(B, D, generator=g).cuda() for _ in range(M)]
    W = (torch.randn(C, M * D, generator=g) * 0.05).cuda()
    b = torch.randn(C, generator=g).cuda()
    label = torch.randint(0, C, (B,), generator=g).cuda()
    out, out_m, loss, loss_m, dl, dW, db, dxs = _ref_head(xs, W, b, label)
    got = T.concat_head_ce_fwd_bwd(xs, W, b, label, 1.0 / B)
    torch.cuda.synchronize()
    names = ("out", "out_m", "loss", "loss_m", "dW", "db")
    for name, g_, w_ in zip(names, got[:6], (out, out_m, loss.reshape(1), loss_m, dW, db)):
        assert_close(g_, w_, atol=2e-5, rtol=1e-5, name=name)
    for m in range(M):
        assert_close(got[6][m], dxs[m], atol=2e-6, rtol=1e-5, name=f"dX_{m}")
    # forward-only and backward-only variants
    f_out, f_out_m = T.concat_head_fwd(xs, W, b)
    assert_close(f_out, out, atol=2e-5, rtol=1e-5, name="fwd out")
    assert_close(f_out_m, out_m, atol=2e-5, rtol=1e-5, name="fwd out_m")
    dlf = dl.float().cuda()
    bw = T.concat_head_bwd(xs, W, dlf * 3.0, 0.5)
    assert_close(bw[0], dW * 1.5, atol=2e-5, rtol=1e-5, name="bwd dW")
    assert_close(bw[1], db * 1.5, atol=2e-6, rtol=1e-5, name="bwd db")
    for m in range(M):
        assert_close(bw[2][m], dxs[m] * 1.5, atol=2e-6, rtol=1e-5, name=f"bwd dX_{m}")
    # bitwise reproducible (no atomics, fixed reduction order)
    again = T.concat_head_ce_fwd_bwd(xs, W, b, label, 1.0 / B)
    for a, c in zip(got[:6], again[:6]):
        assert torch.equal(a, c)
    for a, c in zip(got[6], again[6]):
        assert torch.equal(a, c)


def test_concat_head_bad_label_gives_nan():
    from mla_hip import torch_ops  # noqa: F401
    T = torch.ops.mla_hip
    xs = [torch.randn(4, 512, device="cuda") for _ in range(2)]
    W, b = torch.randn(6, 1024, device="cuda") * 0.05, torch.zeros(6, device="cuda")
    for bad in (6, -1):
        label = torch.tensor([0, 1, bad, 2], device="cuda")
        out, out_m, loss, loss_m, dW, db, dxs = T.concat_head_ce_fwd_bwd(xs, W, b, label, 0.25)
        assert torch.isnan(loss).all() and torch.isnan(loss_m).all()
        assert torch.isfinite(dW).all() and torch.isfinite(out).all()


# ---- fused step vs the reference fixture -------------------------------------------------------------------------------------
class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
    lorb, clip, modal3 = "base", False, False


def _av_state(seed):
    pa, pv = O.make_resnet18_params("audio", seed), O.make_resnet18_params("visual", seed + 1)
    sd = {f"module.audio_net.{k}": v for k, v in pa.items()}
    sd.update({f"module.visual_net.{k}": v for k, v in pv.items()})
    sd.update({f"module.fusion_module.fc_out.{k}": v for k, v in O.make_head_params(1024, 6, seed + 2).items()})
    return sd


def _av_inputs(seed, s, B, spec_hw, T, img_hw):
    spec = O.portable_normal(seed + 100 + s, (B,) + tuple(spec_hw), stream=1, mean=-5.081, std=4.4849)
    image = O.portable_normal(seed + 100 + s, (B, 3, T) + tuple(img_hw), stream=2)
    label = O.portable_labels(seed + 100 + s, B, 6)
    return spec.cuda(), image.cuda(), label.cuda()


def _build_av(seed, modulation, conv_math="f32", alpha=0.3, ge_seed=0):
    from mla_hip import AVClassifier, JointTrainer

    class A(AVArgs):
        pass
    A.modulation = modulation
    model = AVClassifier(A(), seed=0, conv_math=conv_math)
    model.load_state_dict(_av_state(seed))
    tr = JointTrainer(model, lr=1e-3, momentum=0.9, weight_decay=1e-4, modulation=modulation, alpha=alpha, seed=ge_seed)
    return model, tr


@pytest.mark.parametrize("conv_math", ["f32", "split"])
@pytest.mark.parametrize("tag", ["normal", "ogm"])
def test_joint_step_vs_reference_golden(tag, conv_math, golden_dir):
    fx = np.load(os.path.join(golden_dir, "joint_small.npz"))
    B, sh, sw, T, ih, iw, steps, seed = [int(v) for v in fx[f"{tag}.meta"]]
    model, tr = _build_av(seed, str(fx[f"{tag}.modulation"]), conv_math, float(fx[f"{tag}.alpha"]))
    head = model.fusion_module.fc_out
    for s in range(steps):
        spec, image, label = _av_inputs(seed, s, B, (sh, sw), T, (ih, iw))
        losses = tr.train_step(spec, image, label, s)
        torch.cuda.synchronize()
        p = f"{tag}.s{s}."
        tol = TOL if s == 0 else 1e-3          # step 1 is free-running (see test_step_gpu.py)
        for k in ("a", "v", "out"):
            assert_close(tr.last[k], fx[p + k], atol=tol, name=p + k)
        assert_close(tr.last["out_m"][0], fx[p + "out_a"], atol=tol, name=p + "out_a")
        assert_close(tr.last["out_m"][1], fx[p + "out_v"], atol=tol, name=p + "out_v")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), fx[p + k], atol=tol, name=p + k)
        assert_close(head.weight_grad, fx[p + "head_grad"], atol=tol, name=p + "head grad")
        assert_close(head.bias_grad, fx[p + "head_bias_grad"], atol=tol, name=p + "head bias grad")
        if tag == "ogm":
            assert_close(tr.last["coeff"], fx[p + "coeff"], atol=1e-6 if s == 0 else tol, name=p + "coeff")
            assert_close(tr.last["scores"], fx[p + "scores"], atol=1e-5, rtol=1e-5, name=p + "scores")
            assert_close(tr.last["ratios"], fx[p + "ratios"], atol=1e-5, rtol=1e-5, name=p + "ratios")
        sd = model.state_dict()
        assert_close(sd["fusion_module.fc_out.weight"], fx[p + "head.weight"], atol=tol, name=p + "head weight")
        assert_close(sd["fusion_module.fc_out.bias"], fx[p + "head.bias"], atol=tol, name=p + "head bias")
        enc_g = {"audio_net": model.audio_net.grads_as_reference(), "visual_net": model.visual_net.grads_as_reference()}
        for enc in ("audio_net", "visual_net"):
            assert_close(sd[f"{enc}.bn1.running_mean"], fx[p + f"{enc}.bn1.running_mean"], atol=1e-5, rtol=1e-5, name="running_mean")
            assert_close(sd[f"{enc}.bn1.running_var"], fx[p + f"{enc}.bn1.running_var"], atol=1e-5, rtol=1e-5, name="running_var")
            assert_close_robust(sd[f"{enc}.conv1.weight"], fx[p + f"{enc}.conv1.weight"], rel_l2=2e-3, elem_tol=2e-3, frac=0.9,
                                name=f"{p}{enc} conv1.weight")
            w = sd[f"{enc}.layer4.1.conv2.weight"]
            assert_close(w.flatten()[:64], fx[p + f"{enc}.layer4.1.conv2.weight.head"], atol=2e-6, name="layer4 weight slice")
            assert abs(w.double().sum().item() - float(fx[p + f"{enc}.layer4.1.conv2.weight.sum"])) < 1e-3
            # modulated (OGM) encoder gradients: the abs-sum of every kept gradient
            for key in fx.files:
                pre = p + f"grad.{enc}."
                if key.startswith(pre) and key.endswith(".abssum"):
                    name = key[len(pre):-len(".abssum")]
                    g_ = enc_g[enc][name]
                    got = g_.double().abs().sum().item()
                    want = float(fx[key])                 # the gradient loss.backward() left (before the modulation)
                    if tag == "ogm" and g_.dim() == 4:    # OGM scales the conv gradients by the modality's coefficient
                        want *= float(fx[p + "coeff"][0 if enc == "audio_net" else 1])
                    assert abs(got - want) <= 5e-3 * want + 1e-9, f"{key}: {got} vs {want}"
                    head_want = torch.from_numpy(fx[key[:-len(".abssum")] + ".head"]).double() * (want / float(fx[key]))
                    assert_close_robust(g_.flatten()[:64], head_want, rel_l2=5e-2 if s == 0 else 1e-1, elem_tol=1.0, frac=0.0,
                                        name=key[:-len(".abssum")] + ".head")


# ---- the reference's loop verbatim on protocol objects == fused JointTrainer -----------------------------------------------
def _reference_joint_loop(args, model, optimizer, label, epoch, inputs, rec):
    """main.py:130-133, 164-168, 232-237, 273-311, 312-417 verbatim for --lorb base / m3ae (+ --modal3), concat fusion
    (the `rec[...]` lines are the only additions; tensorboard lines left out)."""
    criterion = nn.CrossEntropyLoss()
    softmax = nn.Softmax(dim=1)
    relu = nn.ReLU(inplace=True)
    tanh = nn.Tanh()
    if args.lorb == "m3ae":
        if args.modal3:
            token, padding_mask, image, spec = inputs
        else:
            token, padding_mask, image = inputs
    else:
        spec, image = inputs
    optimizer.zero_grad()
    if args.lorb == "m3ae":
        if args.modal3:
            a, v, t = model(token, padding_mask, image, spec)
            _, _, _, out = model.module.fusion_module(a, v, t)
        else:
            a, v = model(token, padding_mask, image)
            _, _, out = model.module.fusion_module(a, v)
    else:
        a, v, out = model(spec.unsqueeze(1).float(), image.float())
    if args.modal3:
        weight_size = model.module.fusion_module.fc_out.weight.size(1)
        out_t = (torch.mm(t, torch.transpose(model.module.fusion_module.fc_out.weight[:, 2 * weight_size // 3:], 0, 1))
                 + model.module.fusion_module.fc_out.bias / 3)
        out_v = (torch.mm(v, torch.transpose(model.module.fusion_module.fc_out.weight[:, weight_size // 3:2 * weight_size // 3], 0, 1))
                 + model.module.fusion_module.fc_out.bias / 3)
        out_a = (torch.mm(a, torch.transpose(model.module.fusion_module.fc_out.weight[:, :weight_size // 3], 0, 1))
                 + model.module.fusion_module.fc_out.bias / 3)
    else:
        weight_size = model.module.fusion_module.fc_out.weight.size(1)
        out_v = (torch.mm(v, torch.transpose(model.module.fusion_module.fc_out.weight[:, weight_size // 2:], 0, 1))
                 + model.module.fusion_module.fc_out.bias / 2)
        out_a = (torch.mm(a, torch.transpose(model.module.fusion_module.fc_out.weight[:, :weight_size // 2], 0, 1))
                 + model.module.fusion_module.fc_out.bias / 2)
    loss = criterion(out, label)
    if args.modal3:
        loss_t = criterion(out_t, label)
    loss_a = criterion(out_a, label)
    loss_v = criterion(out_v, label)
    loss.backward()
    rec.update(out=out.detach().clone(), loss=loss.detach().clone(), loss_a=loss_a.detach().clone(), loss_v=loss_v.detach().clone())
    if args.modal3:
        rec["loss_t"] = loss_t.detach().clone()
    rec["head_grad"] = model.module.fusion_module.fc_out.weight.grad.detach().clone()
    if args.modulation == 'Normal' or args.modulation == "QMF":
        pass
    else:
        if args.modal3:
            score_v = sum([softmax(out_v)[i][label[i]] for i in range(out_v.size(0))])
            score_a = sum([softmax(out_a)[i][label[i]] for i in range(out_a.size(0))])
            score_t = sum([softmax(out_t)[i][label[i]] for i in range(out_t.size(0))])

            ratio_v = score_v / (score_a + score_t)
            ratio_a = score_a / (score_v + score_t)
            ratio_t = score_t / (score_v + score_a)

            if ratio_v > 1:
                coeff_v = 1 - tanh(args.alpha * relu(ratio_v))
                coeff_a = 1
                coeff_t = 1
            elif ratio_t > 1:
                coeff_t = 1 - tanh(args.alpha * relu(ratio_t))
                coeff_a = 1
                coeff_v = 1
            else:
                coeff_a = 1 - tanh(args.alpha * relu(ratio_a))
                coeff_v = 1
                coeff_t = 1
            rec["coeff"] = (float(coeff_a), float(coeff_v), float(coeff_t))

            if args.modulation_starts <= epoch <= args.modulation_ends:  # bug fixed
                for name, parms in model.named_parameters():
                    if parms.grad is None:
                        continue
                    layer = str(name).split('.')[1]
                    if 'mae_a' in layer and len(parms.grad.size()) == 4:
                        if args.modulation == 'OGM_GE':
                            parms.grad = parms.grad * coeff_a + \
                                torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                        elif args.modulation == 'OGM':
                            parms.grad *= coeff_a

                    if 'mae_v' in layer and len(parms.grad.size()) == 4:
                        if args.modulation == 'OGM_GE':
                            parms.grad = parms.grad * coeff_v + \
                                torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                        elif args.modulation == 'OGM':
                            parms.grad *= coeff_v
                    if 'mae_t' in layer and len(parms.grad.size()) == 4:
                        if args.modulation == 'OGM_GE':
                            parms.grad = parms.grad * coeff_t + \
                                torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                        elif args.modulation == 'OGM':
                            parms.grad *= coeff_t
            else:
                pass
        else:
            score_v = sum([softmax(out_v)[i][label[i]] for i in range(out_v.size(0))])
            score_a = sum([softmax(out_a)[i][label[i]] for i in range(out_a.size(0))])

            ratio_v = score_v / score_a
            ratio_a = 1 / ratio_v

            if ratio_v > 1:
                coeff_v = 1 - tanh(args.alpha * relu(ratio_v))
                coeff_a = 1
            else:
                coeff_a = 1 - tanh(args.alpha * relu(ratio_a))
                coeff_v = 1
            rec["coeff"] = (float(coeff_a), float(coeff_v))

            if args.modulation_starts <= epoch <= args.modulation_ends:  # bug fixed
                for name, parms in model.named_parameters():
                    layer = str(name).split('.')[1]

                    if 'audio' in layer and len(parms.grad.size()) == 4:
                        if args.modulation == 'OGM_GE':
                            parms.grad = parms.grad * coeff_a + \
                                torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                        elif args.modulation == 'OGM':
                            parms.grad *= coeff_a

                    if 'visual' in layer and len(parms.grad.size()) == 4:
                        if args.modulation == 'OGM_GE':
                            parms.grad = parms.grad * coeff_v + \
                                torch.zeros_like(parms.grad).normal_(0, parms.grad.std().item() + 1e-8)
                        elif args.modulation == 'OGM':
                            parms.grad *= coeff_v
            else:
                pass

    optimizer.step()


def _compare_models(m_ref, m_fused, tol_head=1e-5, name="", encoders=True, rel_l2=1e-5, elem_tol=1e-5, frac=0.999):
    sd_r, sd_f = m_ref.state_dict(), m_fused.state_dict()
    for k in ("fusion_module.fc_out.weight", "fusion_module.fc_out.bias"):
        assert_close(sd_f[k], sd_r[k], atol=tol_head, name=f"{name} {k}")
    if not encoders:
        return
    for k in sd_r:
        if k.startswith("fusion_module") or sd_r[k].dtype != torch.float32:
            continue
        assert_close_robust(sd_f[k], sd_r[k], rel_l2=rel_l2, elem_tol=elem_tol, frac=frac, name=f"{name} {k}")


def _loop_case(which, modulation):
    """(protocol model wrapped like main.py:732, fused model, args, inputs on the device, label)"""
    import mla_hip
    if which == "av":
        seed = 31

        class A(AVArgs):
            pass
        A.modulation = modulation
        sd, build = _av_state(seed), (lambda: mla_hip.AVClassifier(A(), seed=0))
        spec, image, label = _av_inputs(seed, 0, 4, (128, 64), 2, (96, 96))
        dev, wrap = [spec, image], torch.nn.DataParallel
        lorb, modal3 = "base", False
    else:
        from test_dist_gpu import T_DEPTH, T_VOCAB, _transformer_case
        A0, sd, inputs, label = _transformer_case(which)
        M = 2 if which == "m3ae" else 3
        C = sd["fusion_module.fc_out.weight"].shape[0]
        sd.update({f"fusion_module.fc_out.{k}": v for k, v in O.make_head_params(768 * M, C, 977).items()})

        class A(A0):
            gs_flag = False
        A.modulation = modulation
        cls = mla_hip.M3AEClassifier if which == "m3ae" else mla_hip.Modal3Classifier
        build = lambda: cls(A(), depth=T_DEPTH, text_vocab_size=T_VOCAB, seed=0)          # noqa: E731
        dev, label, wrap = [x.cuda() for x in inputs], label.cuda(), mla_hip.DataParallel
        lorb, modal3 = "m3ae", which == "modal3"

    class args:
        alpha, modulation_starts, modulation_ends = 0.3, 0, 50
    args.lorb, args.modal3, args.clip, args.modulation = lorb, modal3, False, modulation
    ref = build()
    ref.load_state_dict(sd)
    ref = wrap(ref, device_ids=[0])
    fused = build()
    fused.load_state_dict(sd)
    return ref, fused, args, dev, label


@pytest.mark.parametrize("modulation", ["Normal", "OGM", "OGM_GE"])
@pytest.mark.parametrize("which", ["av", "m3ae", "modal3"])
def test_reference_loop_equals_fused_trainer(which, modulation):
    """The reference's joint loop, OGM / OGM-GE branches included, run on the protocol objects (AV, M3AE and Modal3; Modal3 is
    pinned only by this equality) against JointTrainer from the same state.  Normal and OGM: two steps, everything equal.
    OGM-GE draws torch's normal_() noise in the loop and Philox noise in JointTrainer, so only what the noise cannot reach is
    compared: the first step's outputs, losses and coefficients, and the head after it (its gradients are 2-D: never modulated)."""
    import mla_hip
    ref, fused, args, dev, label = _loop_case(which, modulation)
    optimizer = mla_hip.FusedSGD(ref.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    tr = mla_hip.JointTrainer(fused, lr=1e-3, momentum=0.9, weight_decay=1e-4, modulation=modulation, alpha=args.alpha,
                              modulation_starts=args.modulation_starts, modulation_ends=args.modulation_ends)
    tags = [t for t, _g, _e in fused.mla_encoders()]
    for s in range(1 if modulation == "OGM_GE" else 2):
        rec = {}
        ref.train()
        _reference_joint_loop(args, ref, optimizer, label, s, dev, rec)
        losses = tr.train_step(*dev, label, s)
        torch.cuda.synchronize()
        assert_close(tr.last["out"], rec["out"], atol=1e-5, name=f"{which} s{s} out")
        for k in ["loss"] + ["loss_" + t for t in tags]:
            assert_close(losses[k].reshape(()), rec[k], atol=1e-5, name=f"{which} s{s} {k}")
        if modulation != "Normal":
            assert_close(tr.last["coeff"], torch.tensor(rec["coeff"]), atol=1e-6, name=f"{which} s{s} coeff")
        # step 1 runs from weights that differ in the last bits (the coefficient is torch's tanh on one side, the kernel's on
        # the other; they agree to 1e-6), which can flip a stem ReLU / max-pool decision: measured on the visual stem, relL2
        # 1.9e-5 with 3 % of its elements beyond 1e-5 * max (test_step_gpu.py holds free-running stems to 2e-3 / 90 %)
        _compare_models(ref.module, fused, name=f"{which} {modulation} s{s}", encoders=modulation != "OGM_GE",
                        rel_l2=1e-5 if s == 0 else 1e-4, elem_tol=1e-5 if s == 0 else 1e-4, frac=0.999 if s == 0 else 0.9)
        if modulation == "OGM_GE":          # the loop's modulated gradients were published / copied and applied: finite, moved
            for k, v in ref.module.state_dict().items():
                if v.dtype == torch.float32:
                    assert torch.isfinite(v).all(), k


def test_m3ae_joint_step_vs_reference_golden(golden_dir):
    """--lorb m3ae joint Normal step (depth 2) against the reference encoders + ConcatFusion(1536, 3) (make_golden_joint.py)."""
    from mla_hip import JointTrainer, M3AEClassifier
    fx = np.load(os.path.join(golden_dir, "joint_small.npz"))
    B, depth, vocab, C, steps, seed = [int(v) for v in fx["m3ae.meta"]]

    class A:
        fusion_method, dataset, gs_flag, modulation = "concat", "MVSA", False, "Normal"
    model = M3AEClassifier(A(), depth=depth, text_vocab_size=vocab, seed=0)
    assert model.fusion_module.fc_out.weight.shape == (C, 1536)
    sd = {f"mae_a.{k}": v for k, v in O.make_m3ae_params(seed, depth=depth, vocab=vocab).items()}
    sd.update({f"mae_v.{k}": v for k, v in O.make_m3ae_params(seed + 1, depth=depth, vocab=vocab).items()})
    sd.update({f"fusion_module.fc_out.{k}": v for k, v in O.make_head_params(1536, C, seed + 2).items()})
    model.load_state_dict(sd)
    tr = JointTrainer(model, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    head = model.fusion_module.fc_out
    for s in range(steps):
        token = torch.from_numpy(np.minimum((O.portable_uniform(seed + 50 + s, B * 256, 7) * vocab).astype(np.int64), vocab - 1)).view(B, 1, 256)
        pm = torch.zeros(B, 1, 256)
        for b in range(B):
            pm[b, 0, 40 + 37 * b:] = 1.0
        image = O.portable_normal(seed + 50 + s, (B, 3, 256, 256), stream=3)
        label = O.portable_labels(seed + 50 + s, B, C)
        losses = tr.train_step(token.cuda(), pm.cuda(), image.cuda(), label.cuda(), s)
        torch.cuda.synchronize()
        p = f"m3ae.s{s}."
        tol = TOL if s == 0 else 1e-3
        for k in ("a", "v", "out"):
            assert_close(tr.last[k], fx[p + k], atol=tol, name=p + k)
        assert_close(tr.last["out_m"][0], fx[p + "out_a"], atol=tol, name=p + "out_a")
        assert_close(tr.last["out_m"][1], fx[p + "out_v"], atol=tol, name=p + "out_v")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), fx[p + k], atol=tol, name=p + k)
        assert_close(head.weight_grad, fx[p + "head_grad"], atol=tol, name=p + "head grad")
        assert_close(head.bias_grad, fx[p + "head_bias_grad"], atol=tol, name=p + "head bias grad")
        msd = model.state_dict()
        assert_close(msd["fusion_module.fc_out.weight"], fx[p + "head.weight"], atol=tol, name=p + "head weight")
        assert_close(msd["fusion_module.fc_out.bias"], fx[p + "head.bias"], atol=tol, name=p + "head bias")
        for nm in ("mae_a", "mae_v"):
            assert_close(msd[f"{nm}.cls_token"], fx[p + f"{nm}.cls_token"], atol=1e-6, name=p + f"{nm}.cls_token")
            assert_close(msd[f"{nm}.encoder.blocks.{depth - 1}.transformer_mlp.fc2.weight"].flatten()[:64],
                         fx[p + f"{nm}.fc2w.head"], atol=1e-6, name=p + f"{nm} fc2 weight slice")


def test_overlap_off_is_bitwise_equal_to_overlap_on():
    seed = 41
    res = []
    for overlap in (True, False):
        model, tr = _build_av(seed, "OGM_GE", ge_seed=5)
        tr.set_overlap(overlap)
        for s in range(2):
            spec, image, label = _av_inputs(seed, s, 4, (128, 64), 2, (96, 96))
            tr.train_step(spec, image, label, s)
        torch.cuda.synchronize()
        res.append(model.state_dict())
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


# ---- OGM-GE ---------------------------------------------------------------------------------------------------------------
def test_ogm_ge_reproducible_and_noise_scale():
    seed = 51
    spec, image, label = _av_inputs(seed, 0, 4, (128, 64), 2, (96, 96))
    states = []
    for mode in ("OGM_GE", "OGM_GE", "OGM"):
        model, tr = _build_av(seed, mode, ge_seed=9)
        tr.train_step(spec, image, label, 0)
        torch.cuda.synchronize()
        states.append((model.state_dict(), {e: getattr(model, e).grads_as_reference() for e in ("audio_net", "visual_net")},
                       tr.last["coeff"].clone()))
    (sd1, g1, c1), (sd2, _g2, _c2), (sd3, g3, c3) = states
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), f"OGM_GE with the same seed must be bitwise reproducible: {k}"
    assert torch.equal(c1, c3)
    # the noise OGM_GE adds (main.py:399) = its modulated gradient minus OGM's (coeff * grad), per conv tensor; its std is
    # grad.std() + 1e-8 of the UNSCALED gradient (the weight difference / lr of the first step is the same quantity, but the
    # fp32 weights resolve it too coarsely where the gradient is small)
    checked = 0
    for e, enc_key in (("audio_net", 0), ("visual_net", 1)):
        cf = c3[enc_key].item()
        for k, g_mod in g3[e].items():
            if g_mod.dim() != 4:
                continue
            noise = g1[e][k].double() - g_mod.double()
            want = (g_mod.double() / cf).std().item() + 1e-8
            got = noise.std().item()
            assert abs(got - want) <= 0.05 * want, f"{e}.{k}: noise std {got} vs {want}"
            dw = (sd3[f"{e}.{k}"].double() - sd1[f"{e}.{k}"].double()) / 1e-3
            assert torch.corrcoef(torch.stack([dw.flatten(), noise.flatten()]))[0, 1] > 0.5
            checked += 1
    assert checked == 40


# ---- evaluation -----------------------------------------------------------------------------------------------------------
def test_joint_evaluator_counts(golden_dir):
    from mla_hip import JointEvaluator
    fx = np.load(os.path.join(golden_dir, "joint_small.npz"))
    seed = 7
    model, _tr = _build_av(seed, "Normal")
    ev = JointEvaluator(model)
    num = np.zeros(6)
    acc = np.zeros((3, 6))
    with torch.no_grad():
        for s in range(2):
            spec, image, label = _av_inputs(seed, s, 4, (128, 64), 2, (96, 96))
            out, out_m = ev.update(spec, image, label)
            torch.cuda.synchronize()
            # logits: the head restated in fp64 on the evaluator's own features
            feats = model.forward_raw(spec.unsqueeze(1), image)
            W, b = model.fusion_module.fc_out.weight.detach(), model.fusion_module.fc_out.bias.detach()
            ref = _ref_head(list(feats), W, b, label)
            assert_close(out, ref[0], atol=2e-5, name="eval out")
            assert_close(out_m, ref[1], atol=2e-5, name="eval out_m")
            lab = label.cpu().numpy()
            for k, o in enumerate([out, out_m[0], out_m[1]]):
                pred = np.argmax(o.cpu().numpy(), axis=1)
                for i in range(len(lab)):
                    acc[k, lab[i]] += pred[i] == lab[i]
            for i in range(len(lab)):
                num[lab[i]] += 1
    res = ev.result()
    want = tuple(acc[k].sum() / num.sum() for k in range(3))
    assert res == want, (res, want)
    # counters on the fixture's (reference, train-mode) logits: the counting kernel alone, exactly
    from mla_hip import ops
    counts = torch.zeros(30, dtype=torch.int32, device="cuda")
    expect = np.zeros(30, dtype=np.int64)
    for s in range(2):
        outs = [torch.from_numpy(fx[f"normal.s{s}.{k}"]).cuda() for k in ("out", "out_a", "out_v")]
        lab = O.portable_labels(seed + 100 + s, 4, 6)
        ops.eval_fuse(outs, lab.cuda(), counts, torch.zeros(3, device="cuda"), False, [1.0, 0.0, 0.0])
        for k, o in enumerate(outs):
            pred = np.argmax(o.cpu().numpy(), axis=1)
            for i, l in enumerate(lab.numpy()):
                expect[(2 + k) * 6 + l] += pred[i] == l
                if k == 0:
                    expect[6 + l] += pred[i] == l
                    expect[l] += 1
    assert counts.cpu().numpy().tolist() == expect.tolist()
