"""Whole-step parity: MLATrainer.train_step (HIP) vs the reference's golden outputs and vs the oracle.

Tolerance (BASELINE.json north_star): logits, loss and the projected head gradient within 1e-3
absolute in fp32.  We test tighter: 2e-4 absolute on features/logits/losses/head gradients.  Encoder
gradients and updated encoder weights use the outlier-robust norm-wise check (tests/util.py).
Pinned semantics: projection mode as named per case (Q1); zero_grad = torch>=2 set_to_none unless the
case says "legacy" (Q6).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from util import assert_close, assert_close_robust  # noqa: E402

TOL = 2e-4


def build(seed, gs_mode, legacy, conv_math="f32"):
    from mla_hip import AVClassifier, MLATrainer

    class Args:
        fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"

    model = AVClassifier(Args(), seed=0, conv_math=conv_math)
    pa, pv = O.make_resnet18_params("audio", seed), O.make_resnet18_params("visual", seed + 1)
    hd = O.make_head_params(512, 6, seed + 2)
    sd = {f"module.audio_net.{k}": v for k, v in pa.items()}                    # DataParallel-style keys (main.py:724)
    sd.update({f"module.visual_net.{k}": v for k, v in pv.items()})
    sd.update({f"module.fusion_module.fc_out.{k}": v for k, v in hd.items()})
    model.load_state_dict(sd)
    tr = MLATrainer(model, lr=1e-3, momentum=0.9, weight_decay=1e-4, gs_mode=gs_mode, legacy_zero_grad=legacy)
    tr.keep_debug = True
    st = O.MLAState(pa, pv, hd)
    return model, tr, st


def inputs(seed, s, B, spec_hw, T, img_hw):
    spec = O.portable_normal(seed + 100 + s, (B,) + tuple(spec_hw), stream=1, mean=-5.081, std=4.4849)
    image = O.portable_normal(seed + 100 + s, (B, 3, T) + tuple(img_hw), stream=2)
    label = O.portable_labels(seed + 100 + s, B, 6)
    return spec, image, label


@pytest.mark.parametrize("conv_math", ["f32", "split"])
@pytest.mark.parametrize("tag", ["small_intended", "small_published", "small_legacy", "full_b2"])
def test_step_vs_reference_golden(tag, conv_math, golden_dir):
    fx = np.load(os.path.join(golden_dir, f"mla_{tag}.npz"))
    B, sh, sw, T, ih, iw, steps, seed, ldl = [int(v) for v in fx["meta"]]
    gs_mode, legacy = str(fx["gs_mode"]), bool(int(fx["legacy"]))
    model, tr, _ = build(seed, gs_mode, legacy, conv_math)
    for s in range(steps):
        spec, image, label = inputs(seed, s, B, (sh, sw), T, (ih, iw))
        losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), s, ldl)
        torch.cuda.synchronize()
        # step 0 starts from identical state: 2e-4.  Step 1 is free-running (its weights already contain step 0's
        # flipped ReLU decisions, measured drift 2.3e-4), so it is held to the north-star tolerance 1e-3.
        tol = TOL if s == 0 else 1e-3
        for k in ("a", "v", "out_a", "out_v"):
            assert_close(tr.last[k], fx[f"s{s}.{k}"], atol=tol, name=f"{tag} s{s} {k}")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), fx[f"s{s}.{k}"], atol=tol, name=f"{tag} s{s} {k}")
        assert_close(tr.last["head_grad_a_raw"], fx[f"s{s}.head_grad_a_raw"], atol=tol, name="raw head grad a")
        assert_close(tr.last["head_grad_v_raw"], fx[f"s{s}.head_grad_v_raw"], atol=tol, name="raw head grad v")
        # projected head gradient of the last (visual) phase is still in the head's grad buffer
        assert_close(model.fusion_module.fc_out.weight_grad, fx[f"s{s}.head_grad_v"], atol=tol, name="projected head grad v")
        sd = model.state_dict()
        assert_close(sd["fusion_module.fc_out.weight"], fx[f"s{s}.head.weight"], atol=tol, name="head weight")
        assert_close(sd["fusion_module.fc_out.bias"], fx[f"s{s}.head.bias"], atol=tol, name="head bias")
        for enc in ("audio_net", "visual_net"):
            assert_close(sd[f"{enc}.bn1.running_mean"], fx[f"s{s}.{enc}.bn1.running_mean"], atol=1e-5, rtol=1e-5, name="running_mean")
            assert_close(sd[f"{enc}.bn1.running_var"], fx[f"s{s}.{enc}.bn1.running_var"], atol=1e-5, rtol=1e-5, name="running_var")
            # stem weights after SGD: a single flipped ReLU/max-pool decision between two fp32 evaluation orders
            # (even CPU vs CPU with another thread count) moves this by ~4e-4 relL2 at step 1 -> norm-wise 2e-3
            assert_close_robust(sd[f"{enc}.conv1.weight"], fx[f"s{s}.{enc}.conv1.weight"], rel_l2=2e-3, elem_tol=2e-3, frac=0.9, name=f"{enc} conv1.weight")
            w = sd[f"{enc}.layer4.1.conv2.weight"]
            assert_close(w.flatten()[:64], fx[f"s{s}.{enc}.layer4.1.conv2.weight.head"], atol=2e-6, name="layer4 weight slice")
            assert abs(w.double().sum().item() - float(fx[f"s{s}.{enc}.layer4.1.conv2.weight.sum"])) < 1e-3
        enc_g = {"audio": model.audio_net.grads_as_reference(), "visual": model.visual_net.grads_as_reference()}
        for key in fx.files:
            if key.startswith(f"s{s}.grad.") and key.endswith(".head"):
                _, _, enc, *rest = key.split(".")
                name = ".".join(rest[:-1])
                g = enc_g[enc][name]
                want_abs = float(fx[key[:-5] + ".abssum"])
                got_abs = g.double().abs().sum().item()
                assert abs(got_abs - want_abs) <= 5e-3 * want_abs + 1e-9, f"{key}: abssum {got_abs} vs {want_abs}"
        # Pl digest (as_intended fires from the 2nd before_update call on)
        Pl = tr.gs_plugin.Pl.cpu()
        assert_close(Pl[:8, :8], fx[f"s{s}.Pl.corner"], atol=1e-6, rtol=1e-4, name="Pl corner")
        assert_close(Pl[::16, ::16], fx[f"s{s}.Pl.sub"], atol=1e-6, rtol=1e-4, name="Pl sub")
        assert abs(torch.trace(Pl).item() - float(fx[f"s{s}.Pl.trace"])) < 1e-4


@pytest.mark.parametrize("conv_math", ["f32", "split"])
@pytest.mark.parametrize("B,spec_hw,T,img_hw", [(3, (96, 64), 3, (64, 64)), (8, (256, 128), 3, (112, 112))])
def test_step_vs_oracle_all_grads(B, spec_hw, T, img_hw, conv_math):
    """Every encoder gradient tensor, every updated parameter, BN buffers: HIP vs oracle, 2 steps.

    Two comparisons per step:
      (1) free-running: oracle step vs HIP step.  Features/logits/losses/head gradients element-wise (2e-4).
          Encoder gradients only norm-wise (relL2 <= 5e-2): one ReLU decision that flips under fp32
          re-association (measured: 1 element of layer2.1.bn2.bias) shifts everything downstream by ~1e-3, and
          on the 64x64-frame case layer4 is 2x2 pixels, so one flip moves a layer4 BN-bias gradient by 1-3e-2
          (f32 MFMA: 1.2e-2, split-bf16: 3.2e-2 -- different summation orders flip different decisions).
      After each step the oracle's state is re-synchronised from the HIP state, so step 2 (momentum, fired
      projection, BN running stats) is also compared from an identical start.
      (2) teacher-forced: the oracle's explicit backward is run on the HIP path's own saved forward state
          (same ReLU / max-pool decisions), so EVERY gradient element must agree: 1e-4 * max|ref|.
    """
    from util import oracle_cache_from_hip, sync_oracle_state_from_hip
    seed = 31
    model, tr, st = build(seed, "as_intended", False, conv_math)
    head = model.fusion_module.fc_out
    for s in range(2):
        spec, image, label = inputs(seed, s, B, spec_hw, T, img_hw)
        before = {"audio": {k: v.clone() for k, v in st.audio.items()}, "visual": {k: v.clone() for k, v in st.visual.items()}}
        hip_before = {"audio": {k: v.cpu() for k, v in model.audio_net.state_dict().items()},
                      "visual": {k: v.cpu() for k, v in model.visual_net.state_dict().items()}}
        ref = O.mla_step(st, spec, image, label, s, 10)
        losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), s, 10)
        torch.cuda.synchronize()
        for k in ("a", "v", "out_a", "out_v"):
            assert_close(tr.last[k], ref[k], atol=TOL, name=f"s{s} {k}")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), ref[k], atol=TOL, name=f"s{s} {k}")
        assert_close(head.weight_grad, ref["head_grad_v"], atol=TOL, name="projected head grad")
        for enc, net, slot in (("audio", model.audio_net, "a"), ("visual", model.visual_net, "v")):
            got = net.grads_as_reference()
            # (1) free-running, norm-wise
            for k, want in ref["grads_" + enc].items():
                assert_close_robust(got[k], want, rel_l2=5e-2, elem_tol=1.0, frac=0.0, name=f"s{s} grad {enc}.{k}")
            # (2) teacher-forced, element-wise
            cache = oracle_cache_from_hip(net, hip_before[enc])
            dX = head._bufs(B, slot)["dX"].cpu()
            fshape = cache["layer4.1.out"].shape
            dout = O.audio_pool_bwd(dX, fshape) if enc == "audio" else O.visual_pool_bwd(dX, fshape, B)
            tf = O.resnet18_bwd(hip_before[enc], cache, dout)
            for k, want in tf.items():
                assert_close(got[k], want, atol=1e-7, rtol=1e-4, name=f"s{s} teacher-forced grad {enc}.{k}")
            sd = net.state_dict()
            params = st.audio if enc == "audio" else st.visual
            for k, want in params.items():
                if k.endswith("num_batches_tracked"):
                    assert int(sd[k]) == int(want)
                else:
                    assert_close_robust(sd[k], want, rel_l2=2e-3, elem_tol=1.0, frac=0.0, name=f"s{s} state {enc}.{k}")
        assert_close(tr.gs_plugin.Pl, st.Pl, atol=1e-6, rtol=1e-4, name="Pl")
        assert tr.gs_plugin.exp_count == st.exp_count
        sync_oracle_state_from_hip(st, model, tr)     # next step starts from identical state (momentum, Pl included)


def test_baseline_config0_shapes_bs8():
    """BASELINE.json configs[0] (the reference's CPU-runnable case): CREMA-D shapes -- spec 1x1024x128, 3 frames of
    3x224x224 -- at batch 8, one MLA step from identical state: features, logits, losses, raw and projected head
    gradient against the CPU oracle, both conv arithmetics (the oracle step is computed once)."""
    seed, B = 5, 8
    spec, image, label = inputs(seed, 0, B, (1024, 128), 3, (224, 224))
    ref = None
    for conv_math in ("f32", "split"):
        model, tr, st = build(seed, "as_intended", False, conv_math)
        if ref is None:
            ref = O.mla_step(st, spec, image, label, 0, 100)
        losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), 0, 100)
        torch.cuda.synchronize()
        for k in ("a", "v", "out_a", "out_v"):
            assert_close(tr.last[k], ref[k], atol=TOL, name=f"{conv_math} {k}")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), ref[k], atol=TOL, name=f"{conv_math} {k}")
        assert_close(tr.last["head_grad_a_raw"], ref["head_grad_a_raw"], atol=TOL, name=f"{conv_math} raw head grad a")
        assert_close(model.fusion_module.fc_out.weight_grad, ref["head_grad_v"], atol=TOL, name=f"{conv_math} projected head grad")
        del model, tr
        torch.cuda.empty_cache()


@pytest.mark.parametrize("conv_math", ["f32", "split"])
@pytest.mark.parametrize("B,spec_hw,T,img_hw", [(1, (64, 48), 1, (48, 40)), (5, (130, 70), 2, (70, 50)), (2, (33, 33), 3, (33, 47))])
def test_step_ragged_shapes_and_batch_one(B, spec_hw, T, img_hw, conv_math):
    """Edge shapes: batch 1 (BatchNorm statistics over one sample's pixels), one frame, odd / non-multiple-of-32 spatial
    sizes (every conv, pool and BN kernel on ragged tiles; M far below one workgroup tile in layer4).  One step from
    identical state against the CPU oracle: features, logits, losses, head gradients, BN running statistics."""
    seed = 91
    model, tr, st = build(seed, "as_intended", False, conv_math)
    spec, image, label = inputs(seed, 0, B, spec_hw, T, img_hw)
    ref = O.mla_step(st, spec, image, label, 0, 7)
    losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), 0, 7)
    torch.cuda.synchronize()
    for k in ("a", "v", "out_a", "out_v"):
        assert_close(tr.last[k], ref[k], atol=TOL, rtol=1e-4, name=k)
    for k in ("loss", "loss_a", "loss_v"):
        assert_close(losses[k].reshape(()), ref[k], atol=TOL, name=k)
    assert_close(tr.last["head_grad_a_raw"], ref["head_grad_a_raw"], atol=TOL, rtol=1e-4, name="raw head grad a")
    assert_close(model.fusion_module.fc_out.weight_grad, ref["head_grad_v"], atol=TOL, rtol=1e-4, name="projected head grad v")
    sd = model.state_dict()
    for enc, params in (("audio_net", st.audio), ("visual_net", st.visual)):
        for k in ("bn1.running_mean", "bn1.running_var", "layer4.1.bn2.running_mean", "layer4.1.bn2.running_var"):
            assert_close(sd[f"{enc}.{k}"], params[k], atol=1e-5, rtol=1e-4, name=f"{enc}.{k}")


def test_adjoint_identities_full_size():
    """Size-independent property at the CREMA-D layer shapes (B=64): <dY, conv(X,W)> = <dgrad(dY), X> =
    <wgrad(X,dY), W>.  Exercises the three conv kernels at BASELINE.json's full sizes without a CPU oracle."""
    from mla_hip import ops
    torch.manual_seed(0)
    cases = [(64, 256, 32, 64, 64, 3, 1, 1), (64, 256, 32, 64, 128, 3, 2, 1), (192, 14, 14, 256, 512, 3, 2, 1),
             (192, 7, 7, 512, 512, 3, 1, 1), (64, 128, 16, 128, 256, 1, 2, 0)]
    for (N, H, W, Cin, Cout, k, s, p) in cases:
        x = torch.randn((N, H, W, Cin), device="cuda")
        w = torch.randn((k, k, Cin, Cout), device="cuda") * 0.05
        y, _ = ops.conv2d_fwd(x, w, s, p)
        dy = torch.randn_like(y)
        dx = ops.conv2d_dgrad(dy, w, x.shape, s, p, torch.empty(w.numel(), device="cuda"))
        ws = torch.empty(ops.conv2d_wgrad_ws_bytes(N, H, W, Cin, Cout, k, k, s, p) // 4 + 4, device="cuda")
        dw = ops.conv2d_wgrad(x, dy, torch.empty_like(w), s, p, ws)
        a = (dy.double() * y.double()).sum().item()
        b = (dx.double() * x.double()).sum().item()
        c = (dw.double() * w.double()).sum().item()
        scale = (dy.double().norm() * y.double().norm()).item()
        assert abs(a - b) <= 1e-5 * scale and abs(a - c) <= 1e-5 * scale, (a, b, c, scale)
        # the split-bf16 forward / input-gradient kernels satisfy the same identities at the same sizes
        ys, _ = ops.conv2d_fwd_split(x, ops.conv2d_wsplit(w, True), w.shape, s, p)
        dxs = ops.conv2d_dgrad_split(dy, ops.conv2d_wsplit(w, False), w.shape, x.shape, s, p)
        ws2 = torch.empty(ops.conv2d_wgrad_split_ws_bytes(N, H, W, Cin, Cout, k, k, s, p) // 4 + 4, device="cuda")
        dws = ops.conv2d_wgrad_split(x, dy, torch.empty_like(w), s, p, ws2)
        a2 = (dy.double() * ys.double()).sum().item()
        b2 = (dxs.double() * x.double()).sum().item()
        c2 = (dws.double() * w.double()).sum().item()
        assert abs(a2 - b2) <= 1e-5 * scale and abs(a2 - a) <= 1e-5 * scale and abs(a2 - c2) <= 1e-5 * scale, (a, a2, b2, c2, scale)


def test_loud_failure_without_gpu_library(monkeypatch):
    """The product path has no fallback: a missing libmla_hip.so raises."""
    from mla_hip import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmla_hip.so")
    with pytest.raises(_lib.MLAHipError):
        _lib.load()


def test_rccl_path_single_rank_matches_local():
    """Rehearse the RCCL code path (nccl backend = RCCL) on one GPU: a single-rank process group with
    Comm(force=True) issues the bucketed async encoder-gradient all-reduce and the packed head exchange on
    RCCL's stream; the step must equal the non-distributed step exactly (SUM over one rank = identity)."""
    import socket
    import torch.distributed as dist
    from mla_hip import Comm, MLATrainer
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        seed, B = 41, 4
        model_d, _, _ = build(seed, "as_intended", False)
        tr_d = MLATrainer(model_d, comm=Comm(force=True, bucket_bytes=8 << 20))
        model_l, tr_l, _ = build(seed, "as_intended", False)
        assert tr_d.comm.active and not tr_l.comm.active
        for step in range(3):
            spec, image, label = inputs(seed, step, B, (128, 64), 2, (64, 64))
            ld = tr_d.train_step(spec.cuda(), image.cuda(), label.cuda(), step, 10)
            ll = tr_l.train_step(spec.cuda(), image.cuda(), label.cuda(), step, 10)
            torch.cuda.synchronize()
            for k in ("loss", "loss_a", "loss_v"):
                assert torch.equal(ld[k].cpu(), ll[k].cpu()), k
        assert torch.equal(model_d.audio_net.flat.cpu(), model_l.audio_net.flat.cpu())
        assert torch.equal(model_d.visual_net.flat.cpu(), model_l.visual_net.flat.cpu())
        assert torch.equal(model_d.fusion_module.fc_out.flat.cpu(), model_l.fusion_module.fc_out.flat.cpu())
        assert torch.equal(tr_d.gs_plugin.Pl.cpu(), tr_l.gs_plugin.Pl.cpu())
        # Critical-path cost of the packed head exchange: HIP events on the calling stream around
        # Comm.exchange_head (pack -> all-reduce on the head communicator -> unpack), and the 44.7 MB encoder-gradient
        # all-reduce beside it.  One RCCL rank: the software floor (launches + RCCL kernel), no xGMI wire time.
        import json
        comm, head = tr_d.comm, model_d.fusion_module.fc_out
        colsum, loss, msg = tr_d._colsum, tr_d.losses["loss_a"], tr_d._msg

        def timed(fn, n=50):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / n * 1e3
        us_head = timed(lambda: comm.exchange_head(head.grad, colsum, loss, msg))
        us_enc = timed(lambda: comm.wait(comm.allreduce_flat_async(model_d.audio_net.grad)), n=10)
        rep = {"rccl_ranks": 1, "head_exchange_us": round(us_head, 1), "head_message_floats": int(msg.numel()),
               "encoder_grad_allreduce_us": round(us_enc, 1), "encoder_grad_bytes": int(model_d.audio_net.grad.numel() * 4),
               "bucket_bytes": 8 << 20,
               "note": "single RCCL rank on one MI355X: launch + kernel floor of the two collectives; no multi-GPU box was available"}
        d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "reports")
        os.makedirs(d, exist_ok=True)
        json.dump(rep, open(os.path.join(d, "head_exchange_rccl_1rank.json"), "w"), indent=1)
        assert us_head < 5000
        # The PROTOCOL path (mla_hip.DataParallel: packed dW|db all-reduce inside HeadLinear.backward, asynchronous bucketed
        # encoder-gradient all-reduce awaited by FusedSGD.step(), feature-mean all-reduce in GSPlugin) on the same forced
        # single-rank RCCL group: the reference's loop (main.py:431-476) must give bit-identical parameters with and without it.
        import mla_hip
        from test_protocol_gpu import Args as PArgs, inputs as p_inputs, reference_loop_body

        def protocol_run(comm):
            model, _tr, _ = build(seed, "as_intended", False)
            del _tr
            model = mla_hip.DataParallel(model, device_ids=[0], comm=comm)
            opt = mla_hip.FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
            gs, crit = mla_hip.GSPlugin(), mla_hip.CrossEntropyLoss()
            model.train()
            for step in range(2):
                spec, image, label = p_inputs(seed, step, B, (128, 64), 2, (64, 64))
                opt.zero_grad()
                reference_loop_body(PArgs(), model, opt, gs, crit, spec, image, label, step, 10, 0.55, {}, False)
            torch.cuda.synchronize()
            m = model.module
            return m.audio_net.flat.clone(), m.visual_net.flat.clone(), m.fusion_module.fc_out.flat.clone(), gs.Pl.clone()
        got_d = protocol_run(Comm(force=True, bucket_bytes=8 << 20))
        got_l = protocol_run(Comm())
        for a, b, nm in zip(got_d, got_l, ("audio", "visual", "head", "Pl")):
            assert torch.equal(a, b), f"protocol path over a 1-rank RCCL group changed {nm}"
    finally:
        dist.destroy_process_group()


def test_stream_overlap_is_bitwise_equivalent():
    """The per-encoder stream pipeline (each encoder's forward / backward / SGD on its own stream, weight gradients on
    another, the head path on the caller's stream, chains overlapping across step boundaries) only reorders independent
    kernels: parameters, momentum, Pl and losses after 3 steps equal the serialized trainer's, bit for bit."""
    seed, B = 53, 4
    runs = {}
    for ov in (False, True):
        model, tr, _ = build(seed, "as_intended", False)
        tr.keep_debug = False
        tr.set_overlap(ov)
        assert tr.overlap_forward == ov
        for step in range(3):
            spec, image, label = inputs(seed, step, B, (128, 64), 2, (64, 64))
            losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), step, 10)
        torch.cuda.synchronize()
        runs[ov] = (model.audio_net.flat.cpu(), model.visual_net.flat.cpu(), model.fusion_module.fc_out.flat.cpu(),
                    tr.optimizer.buf["audio"].cpu(), tr.optimizer.buf["visual"].cpu(), tr.gs_plugin.Pl.cpu(),
                    losses["loss"].cpu(), model.audio_net.running.cpu())
    for x, y in zip(runs[False], runs[True]):
        assert torch.equal(x, y)


def test_bn_fold_is_bitwise_equivalent():
    """relu(bn1(.)) folded into conv2's operands (layer1 blocks, encoder.BN_FOLD) is the same arithmetic as the bn_apply pass: three steps give
    bit-identical losses, parameters and running statistics with the fold on and off; the folded blocks exist."""
    from mla_hip import encoder, ops
    seed, B = 59, 4
    runs = {}
    saved, saved_patch = encoder.BN_FOLD, ops.conv2d_patch()
    ops.conv2d_patch(2)          # both runs on the patch kernels (at these sizes the unfolded conv2 would otherwise take the gather-GEMM, which
    try:                         # sums K in another order)
        for fold in (True, False):
            encoder.BN_FOLD = fold
            model, tr, _ = build(seed, "as_intended", False, "split")
            tr.keep_debug = False
            for step in range(3):
                spec, image, label = inputs(seed, step, B, (128, 64), 2, (64, 64))
                losses = tr.train_step(spec.cuda(), image.cuda(), label.cuda(), step, 10)
            torch.cuda.synchronize()
            blocks = [blk for enc in (model.audio_net, model.visual_net) for blk in enc._ws["blocks"]]
            folded = sum(bool(blk["fold"]) for blk in blocks)
            assert all(("a1" in blk) != blk["fold"] for blk in blocks), "relu(bn1(.)) is allocated exactly where it is materialised"
            runs[fold] = (folded, model.audio_net.flat.cpu(), model.visual_net.flat.cpu(), model.fusion_module.fc_out.flat.cpu(),
                          losses["loss"].cpu(), model.audio_net.running.cpu(), model.visual_net.running.cpu())
    finally:
        encoder.BN_FOLD = saved
        ops.conv2d_patch(saved_patch)
    assert runs[True][0] == 4 and runs[False][0] == 0, "layer1's two blocks of both encoders fold, nothing else does"
    for x, y in zip(runs[True][1:], runs[False][1:]):
        assert torch.equal(x, y)


def _audio_encoder_step(enc, x, dfeat, between=None):
    """forward (training mode) -> `between(enc)` -> backward_from_pooled; returns (features, gradient buffer)."""
    enc.train()
    feat = enc.forward(x).clone()
    if between is not None:
        between(enc)
    enc.backward_from_pooled(dfeat, feat.shape[1] * feat.shape[2])
    torch.cuda.synchronize()
    return feat, enc.grad.clone()


def _fold_case(seed):
    """A split-arithmetic audio encoder at B = 4 with the patch kernels forced, so that layer1's blocks fold at this size."""
    from mla_hip.encoder import ResNet18Encoder
    enc = ResNet18Encoder("audio", "cuda", seed=seed, conv_math="split")
    spec = O.portable_normal(seed, (4, 1, 128, 64), stream=1, mean=-5.081, std=4.4849)
    dfeat = O.portable_normal(seed, (4, 512), stream=3)
    return enc, spec.cuda(), dfeat.cuda()


def test_backward_uses_the_fold_plan_of_its_forward():
    """eval() between a folded training forward and its backward does not change the backward: the gradients are bit-identical to those
    of forward -> backward (the backward reads the plan that forward recorded, not the current mode)."""
    from mla_hip import ops
    saved_patch = ops.conv2d_patch()
    ops.conv2d_patch(2)
    try:
        enc, x, dfeat = _fold_case(61)
        feat0, g0 = _audio_encoder_step(enc, x, dfeat)
        assert [blk["fold"] for blk in enc._ws["blocks"]][:2] == [True, True]
        feat1, g1 = _audio_encoder_step(enc, x, dfeat, between=lambda e: e.eval())
    finally:
        ops.conv2d_patch(saved_patch)
    assert torch.equal(feat0, feat1) and torch.equal(g0, g1)


def test_backward_after_an_eval_forward_is_refused():
    """An eval forward overwrites the activations and saves no batch statistics: a backward after it raises instead of reading them."""
    from mla_hip import MLAHipError
    enc, x, dfeat = _fold_case(67)
    enc.forward(x)
    enc.eval()
    feat = enc.forward(x)
    with pytest.raises(MLAHipError, match="eval mode"):
        enc.backward_from_pooled(dfeat, feat.shape[1] * feat.shape[2])
    _audio_encoder_step(enc, x, dfeat)                  # a training forward makes the backward legitimate again
    assert enc.grad_ready


def test_hook_flip_between_steps_is_honoured():
    """ops.conv2d_patch(0) after a folded step (the workspace exists): the next step folds nothing and equals a fresh encoder's step
    with the hook already at 0, bit for bit."""
    from mla_hip import ops
    saved_patch = ops.conv2d_patch()
    try:
        ops.conv2d_patch(2)
        enc, x, dfeat = _fold_case(71)
        _audio_encoder_step(enc, x, dfeat)
        assert any(blk["fold"] for blk in enc._ws["blocks"])
        ops.conv2d_patch(0)
        feat, grad = _audio_encoder_step(enc, x, dfeat)
        assert not any(blk["fold"] for blk in enc._ws["blocks"])
        fresh, _x, _d = _fold_case(71)
        feat_ref, grad_ref = _audio_encoder_step(fresh, x, dfeat)
    finally:
        ops.conv2d_patch(saved_patch)
    assert torch.equal(feat, feat_ref) and torch.equal(grad, grad_ref)


def test_device_feeder_delivers_batches_in_order():
    """SURVEY 8f-2 batch contract: tuples of host tensors (fp32 spec / frames, int64 labels) arrive on the device unchanged
    and in order, also when the consumer lags (slots are recycled only after the consuming step was enqueued)."""
    from mla_hip import DeviceFeeder
    host = [(torch.full((4, 16, 8), float(i)), torch.randn(4, 3, 2, 8, 8) + i, torch.full((4,), i, dtype=torch.int64)) for i in range(7)]
    seen = []
    for i, (spec, image, label) in enumerate(DeviceFeeder(iter(host), depth=3)):
        assert spec.is_cuda and spec.dtype == torch.float32 and label.dtype == torch.int64
        y = (spec.sum() + image.sum()).item() if i % 2 else None      # sometimes force a sync, sometimes run ahead
        seen.append((spec.clone(), image.clone(), label.clone()))
    torch.cuda.synchronize()
    assert len(seen) == 7
    for (s, im, l), (hs, him, hl) in zip(seen, host):
        assert torch.equal(s.cpu(), hs) and torch.equal(im.cpu(), him) and torch.equal(l.cpu(), hl)


def test_full_size_config1_step_properties():
    """BASELINE configs[1] at its real size (CREMA-D shapes, batch 64) through whole steps, without a CPU oracle:
    (1) the per-encoder stream pipeline equals the serialized trainer bit for bit after two steps;
    (2) the two conv arithmetics agree on the north-star outputs of step 0 (logits, loss, raw and projected head gradient)
        within 2e-4 -- they share nothing but the inputs, and each is pinned to the CPU oracle at batch 8 / 2;
    (3) BatchNorm statistics, losses and parameters stay finite."""
    seed, B = 7, 64
    spec0, image0, label0 = [x.cuda() for x in inputs(seed, 0, B, (1024, 128), 3, (224, 224))]
    spec1, image1, label1 = [x.cuda() for x in inputs(seed, 1, B, (1024, 128), 3, (224, 224))]
    out = {}
    for name, conv_math, overlap in (("f32_overlap", "f32", True), ("f32_serial", "f32", False), ("split_overlap", "split", True)):
        model, tr, _ = build(seed, "as_intended", False, conv_math)
        tr.set_overlap(overlap)
        l0 = {k: v.clone() for k, v in tr.train_step(spec0, image0, label0, 0, 100).items()}
        rec = {"out_a": tr.last["out_a"].clone(), "out_v": tr.last["out_v"].clone(), "raw_a": tr.last["head_grad_a_raw"].clone(),
               "proj_v": tr.last["head_grad_v"].clone(), "loss0": l0}
        l1 = tr.train_step(spec1, image1, label1, 1, 100)
        tr.join()
        torch.cuda.synchronize()
        rec.update(loss1={k: v.clone() for k, v in l1.items()}, audio=model.audio_net.flat.clone(), visual=model.visual_net.flat.clone(),
                   head=model.fusion_module.fc_out.flat.clone(), Pl=tr.gs_plugin.Pl.clone(), running=model.visual_net.running.clone(),
                   mom=tr.optimizer.buf["visual"].clone())
        out[name] = rec
        for k in ("audio", "visual", "head", "Pl", "running", "mom"):
            assert torch.isfinite(rec[k]).all(), (name, k)
        assert (model.visual_net.running[model.visual_net._tot_bn:] > 0).all()          # running_var stays positive
        del model, tr
        torch.cuda.empty_cache()
    a, b = out["f32_overlap"], out["f32_serial"]
    for k in ("audio", "visual", "head", "Pl", "running", "mom", "out_a", "out_v", "proj_v"):
        assert torch.equal(a[k], b[k]), f"stream pipeline changed {k}"
    assert all(torch.equal(a["loss1"][k], b["loss1"][k]) for k in a["loss1"])
    c = out["split_overlap"]
    for k in ("out_a", "out_v", "raw_a", "proj_v"):
        assert_close(c[k], a[k], atol=TOL, name=f"f32 vs split {k} (B=64)")
    for k in ("loss", "loss_a", "loss_v"):
        assert_close(c["loss0"][k], a["loss0"][k], atol=TOL, name=f"f32 vs split {k} (B=64)")


def test_device_feeder_with_stream_pipeline_is_bitwise_equivalent():
    """the feeder recycles a device slot as soon as the consuming step has been ENQUEUED on the caller's
    stream, while the overlapped trainer's encoder chains (stem weight gradient reading the spectrogram) are still running
    on their own streams.  Drive DeviceFeeder(depth=3) + the stream pipeline for 6 steps with distinct batches and no
    host synchronisation, and compare with the serialized trainer fed from plain device tensors: bit for bit."""
    from mla_hip import DeviceFeeder
    seed, B, steps = 67, 4, 6
    host = []
    for s in range(steps):
        spec, image, label = inputs(seed, s, B, (128, 64), 2, (64, 64))
        host.append((spec.pin_memory(), image.pin_memory(), label.pin_memory()))
    model_s, tr_s, _ = build(seed, "as_intended", False)
    tr_s.keep_debug = False
    tr_s.set_overlap(False)
    for s, (spec, image, label) in enumerate(host):
        tr_s.train_step(spec.cuda(), image.cuda(), label.cuda(), s, 10)
    torch.cuda.synchronize()
    model_f, tr_f, _ = build(seed, "as_intended", False)
    tr_f.keep_debug = False
    assert tr_f.overlap_forward
    for s, (spec, image, label) in enumerate(DeviceFeeder(iter(host), depth=3)):
        tr_f.train_step(spec, image, label, s, 10)                         # no .item(), no synchronize between steps
    tr_f.join()
    torch.cuda.synchronize()
    for a, b in ((model_s.audio_net.flat, model_f.audio_net.flat), (model_s.visual_net.flat, model_f.visual_net.flat),
                 (model_s.fusion_module.fc_out.flat, model_f.fusion_module.fc_out.flat), (tr_s.gs_plugin.Pl, tr_f.gs_plugin.Pl),
                 (tr_s.optimizer.buf["audio"], tr_f.optimizer.buf["audio"])):
        assert torch.equal(a, b)


def test_training_learns_a_synthetic_task():
    """End to end, beyond step parity: 100 MLA steps on a learnable synthetic task (the label shifts the spectrogram mean and
    tints the frames) with the shipped defaults (split arithmetic, stream pipeline, projection as_intended).  The trajectory is
    spiky -- the CPU oracle on the same data shows the same spikes (scripts/learn_probe.py: HIP and oracle agree to 3 digits for
    ~15 steps, then drift apart chaotically but stay alike) -- so windows are compared: the median loss of the last 40 steps must
    be well below the first steps' (chance: ln 6 = 1.79), everything stays finite, the projector has fired."""
    from mla_hip import AVClassifier, MLATrainer
    model = AVClassifier(type("A", (), dict(fusion_method="concat", dataset="CREMAD", gs_flag=True, modulation="Normal"))(), seed=3)
    tr = MLATrainer(model, lr=3e-3, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator(device="cuda").manual_seed(0)
    B, steps = 16, 100
    hist = []
    for s in range(steps):
        label = torch.randint(0, 6, (B,), device="cuda", generator=g)
        spec = torch.randn((B, 128, 64), device="cuda", generator=g) + (label.float() - 2.5)[:, None, None] * 0.8
        image = torch.randn((B, 3, 2, 64, 64), device="cuda", generator=g)
        image[:, 0] += (label.float() - 2.5)[:, None, None, None] * 0.6
        image[:, 1] -= (label.float() % 2)[:, None, None, None] * 0.8
        losses = tr.train_step(spec, image, label, s % 10, 10)
        hist.append(torch.stack([losses["loss_a"].reshape(()), losses["loss_v"].reshape(())]).clone())     # stays on the device
    tr.join()
    hist = torch.stack(hist).cpu()
    assert torch.isfinite(hist).all()
    head, tail = hist[:3].mean(0), hist[60:].median(0).values          # median: single-step spikes of 5-10 are part of this training
    assert (head > 1.2).all(), head
    assert (tail < 0.6 * head).all(), (head, tail)
    assert tr.gs_plugin.exp_count == 2 * steps and not torch.equal(tr.gs_plugin.Pl.cpu(), torch.eye(512))
    assert torch.isfinite(model.audio_net.flat).all() and torch.isfinite(model.visual_net.flat).all()


def test_streams_on_distinct_hardware_queues():
    """mla_hip.streams: ROCm multiplexes HIP streams onto a few hardware queues and two streams on one queue serialise, so the
    stream pipeline used to keep or lose its overlap with the number of streams the process had created before (two extra
    streams: both encoder chains on one queue, +11 % step time).  distinct_streams measures the sharing with spin kernels: the
    streams it hands out for the encoder chains must not serialise with each other nor with the current stream, whatever was
    created first."""
    from mla_hip import streams
    dev = torch.device("cuda")
    junk = [torch.cuda.Stream() for _ in range(2)]                 # what RCCL / a second model / a loader would do
    for st in junk:
        with torch.cuda.stream(st):
            torch.zeros(16, device=dev).add_(1)
    got = streams.distinct_streams(4, dev)
    assert len(got) == 4
    pool = streams._pools[torch.cuda.current_device()]
    assert len(pool.classes) >= 3, "expected at least three hardware queues besides the caller's"
    cur = torch.cuda.current_stream()
    assert not pool.shares_queue(got[0], got[1]), "the two encoder-chain streams share a hardware queue"
    assert not pool.shares_queue(cur, got[0]) and not pool.shares_queue(cur, got[1])
    assert not pool.shares_queue(got[0], got[2]) and not pool.shares_queue(got[1], got[2])
    again = streams.distinct_streams(2, dev)                        # drawn from the same pool
    assert again[0] is got[0] and again[1] is got[1]
