"""FusedAdam in protocol mode on a depth-1 CAVClassifier against torch.optim.Adam on cloned CPU parameters, identical injected
gradients.

Tolerances.  Parameters 1e-6 absolute (|p| <= a few, so a handful of fp32 ulps over four steps; an Adam step is at most about lr).
exp_avg 1e-5 and exp_avg_sq 5e-5 relative to the tensor's largest element: the C ABI carries beta2 as fp32, so 1 - beta2 is
1.3e-5 (relative) off torch's double -- in exp_avg_sq and in its bias correction alike, which is why the parameters do not see it
(include/mla_hip.h)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from util import assert_close  # noqa: E402

LR, BETAS, WD = 1e-3, (0.95, 0.999), 5e-7
MLP_LIST = ["fusion_module.fc_out.weight", "module.fusion_module.fc_out.bias"]      # main.py:739, typo included


class Args:
    fusion_method, dataset, gs_flag, modulation, lorb = "concat", "CREMAD", True, "Normal", "large"


def make():
    """(model, names, CPU clones of its parameters) -- a fresh model per test: the optimiser changes it."""
    from mla_hip import CAVClassifier
    model = CAVClassifier(Args(), depth=1, seed=4)
    named = list(model.named_parameters())
    return model, [n for n, _p in named], [p.detach().cpu().clone().requires_grad_(True) for _n, p in named]


def torch_groups(names, cpu, lr=LR):
    """main.py:739-745 over the clones."""
    return [{"params": [p for n, p in zip(names, cpu) if n not in MLP_LIST], "lr": lr / 10},
            {"params": [p for n, p in zip(names, cpu) if n in MLP_LIST], "lr": lr}]


def state_index(names):
    """name -> index in an optimiser state_dict: torch numbers the parameters group by group (base group first)."""
    order = [n for n in names if n not in MLP_LIST] + [n for n in names if n in MLP_LIST]
    return {n: i for i, n in enumerate(order)}


def inject(model, cpu, names, seed: int, skip=(), value=None):
    """The same gradient on both sides: N(0, 1) * 1e-2 per parameter (or `value` everywhere); parameters under `skip` get None."""
    gen = torch.Generator().manual_seed(seed)
    for (n, p), c in zip(model.named_parameters(), cpu):
        if n.startswith(tuple(skip)) if skip else False:
            p.grad, c.grad = None, None
            continue
        g = torch.full(c.shape, value) if value is not None else torch.randn(c.shape, generator=gen) * 1e-2
        c.grad = g
        p.grad = g.cuda()


def compare(model, opt, cpu, topt, names, what=""):
    torch.cuda.synchronize()
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert set(sd["state"]) == set(tsd["state"]), f"{what}: which parameters carry state"
    index = state_index(names)
    for (n, p), c in zip(model.named_parameters(), cpu):
        i = index[n]
        assert_close(p.detach(), c.detach(), atol=1e-6, name=f"{what} {n}")
        if i in tsd["state"]:
            s, t = sd["state"][i], tsd["state"][i]
            assert float(s["step"]) == float(t["step"]), (what, n, float(s["step"]), float(t["step"]))
            assert s["exp_avg"].shape == t["exp_avg"].shape == c.shape
            assert_close(s["exp_avg"], t["exp_avg"], atol=0.0, rtol=1e-5, name=f"{what} exp_avg {n}")
            assert_close(s["exp_avg_sq"], t["exp_avg_sq"], atol=0.0, rtol=5e-5, name=f"{what} exp_avg_sq {n}")


def pair(model, names, cpu, lr=LR):
    from mla_hip import FusedAdam, cav_param_groups
    return (FusedAdam(cav_param_groups(model, lr), betas=BETAS, weight_decay=WD),
            torch.optim.Adam(torch_groups(names, cpu, lr), betas=BETAS, weight_decay=WD))


def test_per_owner_step_counters_match_torch():
    """Four steps; the visual encoder's gradients are None on steps 2 and 3: it is skipped without its counter advancing (torch's
    per-parameter rule), so it ends at step 2 while the head and the audio encoder end at 4."""
    model, names, cpu = make()
    opt, topt = pair(model, names, cpu)
    for k in range(4):
        inject(model, cpu, names, 100 + k, skip=("mae_v.",) if k in (1, 2) else ())
        opt.step()
        topt.step()
        compare(model, opt, cpu, topt, names, f"step {k + 1}")
    assert opt.steps == {"SharedHead0": 4, "M3AEEncoder1": 4, "M3AEEncoder2": 2}
    sd = opt.state_dict()
    steps = {n: float(sd["state"][i]["step"]) for n, i in state_index(names).items()}
    assert steps["mae_v.norm_v.weight"] == 2 and steps["mae_a.norm_a.weight"] == 4 and steps["fusion_module.fc_out.bias"] == 4


def test_partial_gradients_inside_one_owner():
    """One parameter of an owner without a gradient: the owner is stepped in runs, that parameter's counter stays behind, and once it
    catches up in count it still differs in history -- parameters and state keep matching torch's."""
    model, names, cpu = make()
    opt, topt = pair(model, names, cpu)
    for k in range(3):
        inject(model, cpu, names, 200 + k, skip=("mae_a.pos_embed_a",) if k == 1 else ())
        opt.step()
        topt.step()
        compare(model, opt, cpu, topt, names, f"step {k + 1}")
    seg = opt.seg_steps["M3AEEncoder1"]
    assert seg is not None and sorted(set(seg)) == [2, 3]


def test_cav_param_groups_lr_against_lr_over_ten():
    """All-ones gradients, one step: Adam moves every element by lr * 1 / (1 + eps) of its group (+ the weight decay's share), so
    the head's weight (lr) moves ten times as far as its bias (lr / 10, the reference's name typo, main.py:739)."""
    model, names, cpu = make()
    head = model.fusion_module.fc_out
    w0, b0 = head.weight.detach().clone(), head.bias.detach().clone()
    opt, topt = pair(model, names, cpu)
    inject(model, cpu, names, 0, value=1.0)
    opt.step()
    topt.step()
    compare(model, opt, cpu, topt, names, "ones")
    dw, db = (w0 - head.weight.detach()).mean().item(), (b0 - head.bias.detach()).mean().item()
    assert abs(dw / LR - 1) < 1e-3 and abs(db / (LR / 10) - 1) < 1e-3 and abs(dw / db - 10) < 1e-2, (dw, db)
    assert [len(g["params"]) for g in opt.param_groups] == [len(names) - 1, 1]


def test_multisteplr_schedules_both_alike():
    """--cav_lrs (main.py:751-757): MultiStepLR(range(2, 1000), 0.5) through param_groups."""
    model, names, cpu = make()
    opt, topt = pair(model, names, cpu)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, list(range(2, 1000, 1)), gamma=0.5)
    tsch = torch.optim.lr_scheduler.MultiStepLR(topt, list(range(2, 1000, 1)), gamma=0.5)
    seen = []
    for epoch in range(4):
        inject(model, cpu, names, 300 + epoch)
        opt.step()
        topt.step()
        sch.step()
        tsch.step()
        lrs, tlrs = [g["lr"] for g in opt.param_groups], [g["lr"] for g in topt.param_groups]
        assert lrs == tlrs
        seen.append(lrs)
        compare(model, opt, cpu, topt, names, f"epoch {epoch}")
    assert seen == [pytest.approx([LR / 10 / f, LR / f], rel=1e-12) for f in (1, 2, 4, 8)]


def test_state_dict_to_torch_and_back():
    model, names, cpu = make()
    opt, topt = pair(model, names, cpu)
    for k in range(2):
        inject(model, cpu, names, 400 + k, skip=("mae_v.",) if k == 1 else ())
        opt.step()
        topt.step()
    torch.cuda.synchronize()
    # ours -> a fresh torch.optim.Adam over the clones
    topt2 = torch.optim.Adam(torch_groups(names, cpu), betas=BETAS, weight_decay=WD)
    topt2.load_state_dict(opt.state_dict())
    # torch's -> a fresh FusedAdam over the model
    opt2, _ = pair(model, names, cpu)
    opt2.load_state_dict(topt.state_dict())
    assert opt2.steps == {"SharedHead0": 2, "M3AEEncoder1": 2, "M3AEEncoder2": 1}
    inject(model, cpu, names, 402)
    opt2.step()
    topt2.step()
    compare(model, opt2, cpu, topt2, names, "after the round trip")


def test_foreign_tensor_raises():
    from mla_hip import FusedAdam, MLAHipError
    model, _names, _cpu = make()
    with pytest.raises(MLAHipError, match="FusedAdam drives mla_hip parameters only"):
        FusedAdam(list(model.parameters()) + [torch.zeros(3, device="cuda", requires_grad=True)])


def test_legacy_zero_grad_still_decays_and_applies_weight_decay():
    """zero_grad(set_to_none=False), torch 1.8.1's behaviour: the gradients stay as zero-filled tensors, so the next
    step() still decays m and v, applies the weight decay and moves the parameters along the decayed m."""
    model, names, cpu = make()
    from mla_hip import FusedAdam, cav_param_groups
    opt = FusedAdam(cav_param_groups(model, LR), betas=BETAS, weight_decay=1e-3)
    topt = torch.optim.Adam(torch_groups(names, cpu), betas=BETAS, weight_decay=1e-3)
    inject(model, cpu, names, 500)
    opt.step()
    topt.step()
    before = model.mae_a.flat.clone()
    m_before = opt.m["M3AEEncoder1"].clone()
    opt.zero_grad(set_to_none=False)
    topt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not p.grad.any() for p in model.mae_a.parameters())
    opt.step()
    topt.step()
    compare(model, opt, cpu, topt, names, "zeroed gradients")
    assert not torch.equal(model.mae_a.flat, before) and opt.steps["M3AEEncoder1"] == 2
    ratio = (opt.m["M3AEEncoder1"].norm() / m_before.norm()).item()
    assert 0.94 < ratio < 0.96, ratio                        # m <- 0.95 m + 0.05 * wd * p: wd p is small against m here
