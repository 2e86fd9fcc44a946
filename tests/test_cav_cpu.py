"""CPU: constructor-level checks of the `--lorb large` family (CAVClassifier, cav_param_groups), the host state machine of FusedAdam
on stand-in owners, and mla_adam_step's argument checks (validation fails before any launch: no GPU, pointers never dereferenced)."""
import ctypes

import pytest
import torch

import cav_model as C


class Args:
    fusion_method, dataset, gs_flag, modulation, lorb = "concat", "CREMAD", True, "Normal", "large"


def test_cav_classifier_keys_and_shapes_cpu():
    from mla_hip import CAVClassifier
    m = CAVClassifier(Args(), device="cpu", depth=2, seed=0)
    sd = m.state_dict()
    assert list(sd) == C.classifier_keys(2)
    want = {**{"mae_v." + k: tuple(v.shape) for k, v in C.make_visual_params(1, depth=2).items()},
            "fusion_module.fc_out.weight": (6, 768), "fusion_module.fc_out.bias": (6,), "mae_a.patch_embed_a.proj.weight": (768, 1, 16, 16),
            "mae_a.pos_embed_a": (1, 512, 768), "mae_a.blocks_u.0.norm1_a.weight": (768,), "mae_a.blocks_a.0.attn.qkv.weight": (2304, 768)}
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    assert sd["mae_v.patch_embed_v.proj.weight"].shape == (768, 3, 16, 16) and sd["mae_v.pos_embed_v"].shape == (1, 196, 768)
    # the visual position embedding starts as get_2d_sincos_pos_embed(768, 14, 14) (cav_mae.py:164): first row sin(0) / cos(0)
    pe = sd["mae_v.pos_embed_v"][0]
    assert torch.equal(pe[0, :192], torch.zeros(192)) and torch.equal(pe[0, 192:384], torch.ones(192))
    assert not torch.equal(pe[1], pe[14]) and pe.abs().max() <= 1
    # the patch weight is a view of the flat buffer in the kernels' [(c, ph, pw)][D] layout
    w = m.mae_v.patch_embed_v.proj.weight
    assert w.untyped_storage().data_ptr() == m.mae_v.flat.untyped_storage().data_ptr()
    with torch.no_grad():
        w[5, 2, 3, 7] = 42.0
    assert m.mae_v.p["patch_embed_v.proj.weight"][2 * 256 + 3 * 16 + 7, 5] == 42.0
    # depth 12: 11 modality blocks + the shared one, per branch (cav_mae.py:138-140)
    full = C.classifier_keys(12)
    assert "mae_v.blocks_v.10.mlp.fc2.bias" in full and "mae_v.blocks_u.0.norm2_v.weight" in full and "mae_v.blocks_v.11.norm1.weight" not in full
    # without --gs_flag: Linear(1536, 6) on cat(a, v) (basic_model.py:98)
    class J(Args):
        gs_flag = False
    assert CAVClassifier(J(), device="cpu", depth=1, seed=0).fusion_module.fc_out.weight.shape == (6, 1536)


def test_cav_classifier_error_behaviour_cpu():
    from mla_hip import AVClassifier, CAVClassifier

    class Bad(Args):
        dataset = "AVE"
    with pytest.raises(NotImplementedError, match="Incorrect dataset name AVE"):           # basic_model.py:90
        CAVClassifier(Bad(), device="cpu", depth=1)

    class Sum(Args):
        fusion_method = "sum"
    with pytest.raises(NotImplementedError, match="Incorrect fusion method: sum!"):        # basic_model.py:104
        CAVClassifier(Sum(), device="cpu", depth=1)

    class Joint(Args):
        gs_flag = False
    with pytest.raises(NotImplementedError, match="large"):                                # the ResNet family stays as it was
        AVClassifier(Joint(), device="cpu")


def test_cav_param_groups_membership_cpu():
    from mla_hip import CAVClassifier, FusedAdam, cav_param_groups
    m = CAVClassifier(Args(), device="cpu", depth=1, seed=0)
    base, head = cav_param_groups(m, 1e-3)
    assert base["lr"] == 1e-4 and head["lr"] == 1e-3
    fc = m.fusion_module.fc_out
    assert len(head["params"]) == 1 and head["params"][0] is fc.weight
    assert any(p is fc.bias for p in base["params"]), "main.py:739 names 'module.fusion_module.fc_out.bias': the bias stays in the base group"
    names = [n for n, _p in m.named_parameters()]
    assert (len(base["params"]), len(head["params"])) == tuple(len(x) for x in C.cav_group_names(names))
    opt = FusedAdam([base, head], betas=(0.95, 0.999), weight_decay=5e-7)
    assert list(opt.groups) == ["SharedHead0", "M3AEEncoder1", "M3AEEncoder2"]
    hy = opt._hypers("SharedHead0")                                  # per registered parameter: weight, bias
    assert hy == [(1e-3, 0.95, 0.999, 1e-8, 5e-7), (1e-4, 0.95, 0.999, 1e-8, 5e-7)]
    assert len(set(opt._hypers("M3AEEncoder1"))) == 1               # uniform owner: one launch
    sch = torch.optim.lr_scheduler.StepLR(opt, 1, 0.1)
    opt.step()                                                       # no gradients anywhere: nothing is launched
    sch.step()
    assert opt._hypers("SharedHead0")[0][0] == pytest.approx(1e-4) and opt._hypers("SharedHead0")[1][0] == pytest.approx(1e-5)


def test_fused_adam_state_machine_cpu(monkeypatch):
    """Trainer mode on stand-in owners (as test_abi.py does for FusedSGD): which launches happen, with which step number."""
    from mla_hip import FusedAdam, MLAHipError, ops

    class G:
        def __init__(self):
            self.flat, self.grad = torch.zeros(8), torch.zeros(8)
    calls = []
    monkeypatch.setattr(ops, "adam_step", lambda p, g, m, v, lr, b1, b2, eps, wd, step: calls.append((g is not None, lr, step)))
    for legacy, want in ((False, "none"), (True, "zero")):
        opt = FusedAdam({"audio": G(), "visual": G(), "head": G()}, lr=1e-3, legacy_zero_grad=legacy)
        opt.mark_ready("audio")
        opt.zero_grad()
        assert opt.grad_state["audio"] == want and opt.grad_state["visual"] == "none"     # Q6
        opt.drop_grads()
        assert set(opt.grad_state.values()) == {"none"}
    # one MLA iteration: head stepped in both phases, each encoder once; "none" groups are skipped and do not count
    opt = FusedAdam({"audio": G(), "visual": G(), "head": G()}, lr=1e-3)
    for it in range(2):
        opt.zero_grad()
        for enc in ("audio", "visual"):
            opt.mark_ready("head")
            opt.step_group("head")
            opt.mark_ready(enc)
            opt.step_group(enc)
        opt.step_group("visual")                                   # still "ready": a second step, as torch would take it
        opt.drop_grads()
        opt.step()                                                 # everything "none": nothing happens
    assert opt.steps == {"audio": 2, "visual": 4, "head": 4}
    assert [c[2] for c in calls] == [1, 1, 2, 1, 2, 3, 2, 4, 3, 4] and all(c[0] for c in calls)
    # legacy zero_grad: a "zero" group is launched without a gradient and still counts a step
    calls.clear()
    opt = FusedAdam({"audio": G(), "head": G()}, lr=1e-3, legacy_zero_grad=True)
    opt.mark_ready("audio")
    opt.step_group("audio")
    opt.zero_grad()
    opt.step_group("audio")
    assert calls == [(True, 1e-3, 1), (False, 1e-3, 2)]
    # a per-owner lr mapping must name every owner
    with pytest.raises(MLAHipError, match="lacks the owners"):
        FusedAdam({"audio": G(), "head": G()}, lr={"audio": 1e-4})
    with pytest.raises(MLAHipError, match="FusedAdam drives mla_hip parameters only"):
        FusedAdam([torch.zeros(3, requires_grad=True)])


def test_fused_adam_per_owner_lr_mapping_cpu(monkeypatch):
    from mla_hip import CAVClassifier, FusedAdam, ops
    m = CAVClassifier(Args(), device="cpu", depth=1, seed=0)
    calls = []
    monkeypatch.setattr(ops, "adam_step", lambda p, g, mm, v, lr, b1, b2, eps, wd, step: calls.append((p.numel(), lr, step)))
    head = m.fusion_module.fc_out
    opt = FusedAdam({"audio": m.mae_a, "visual": m.mae_v, "head": head}, lr={"audio": 1e-4, "visual": 2e-4, "head": 1e-3}, weight_decay=5e-7)
    for k in ("audio", "visual", "head"):
        opt.mark_ready(k)
    opt.step()
    assert calls == [(m.mae_a.numel, 1e-4, 1), (m.mae_v.numel, 2e-4, 1), (head.numel, 1e-3, 1)]      # uniform owners: one launch each
    # the reference's groups: the head splits into weight (lr) and bias (lr / 10), adjacent ranges of equal hyper-parameters merge
    from mla_hip import cav_param_groups
    calls.clear()
    opt = FusedAdam({"audio": m.mae_a, "visual": m.mae_v, "head": head}, param_groups=cav_param_groups(m, 1e-3), weight_decay=5e-7)
    opt.mark_ready("head")
    opt.step_group("head")
    opt.step_group("head")
    assert calls == [(6 * 768, 1e-3, 1), (6, 1e-4, 1), (6 * 768, 1e-3, 2), (6, 1e-4, 2)] and opt.steps["head"] == 2


def test_adam_step_rejects_bad_arguments_before_launch():
    from mla_hip import _lib
    lib = _lib.load()
    fake = 0x1000                                       # non-null, 16-byte aligned, never dereferenced
    call = lambda p, g, m, v, n, step: lib.mla_adam_step(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, None)
    assert call(None, fake, fake, fake, 8, 1) == -1 and b"null pointer" in lib.mla_last_error()
    assert call(fake, fake, None, fake, 8, 1) == -1
    assert call(fake, fake, fake, None, 8, 1) == -1
    assert call(fake, fake, fake, fake, 0, 1) == -1 and b"n == 0" in lib.mla_last_error()
    assert call(fake, fake, fake, fake, 8, 0) == -1 and b"step must be >= 1" in lib.mla_last_error()
    assert call(fake, fake, fake, fake, 8, -3) == -1
    assert call(fake + 2, fake, fake, fake, 8, 1) == -1 and b"4-byte aligned" in lib.mla_last_error()
    assert hasattr(torch.ops.mla_hip, "adam_step")
    import mla_hip.torch_ops as T
    assert "adam_step" in T.op_names()
    with pytest.raises(Exception):                      # no CPU implementation: torch's "no kernel" error
        z = torch.zeros(4)
        torch.ops.mla_hip.adam_step(z, z, z, z, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
