"""GPU: the `--clip` model -- the fused head-only phase (csrc/feature_step.hip) against the general chain and the CPU oracle, the
trainers and evaluators on CLIPClassifier against the reference fixture and the restatement in tests/clip_model.py, and the
device-resident batch feed.

The fused phase carries the projection in fp64, the chain in fp32: the two agree to the tolerances, not bit for
bit, except in logits and loss.  Tolerances of the phase are the ones tests/test_ops_gpu.py holds the chain's kernels to: logits / loss 2e-6 + 2e-6 rel; Pl, W and
momentum where projected 1e-8 + 2e-5 rel; unprojected W, b, momentum 1e-7 + 1e-6 rel."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from util import assert_close  # noqa: E402
import clip_model as R  # noqa: E402

LR, MOM, WD = 1e-3, 0.9, 1e-4
TOL = 2e-4            # tests/test_step_gpu.py: step 0 against a reference fixture; free-running steps 1e-3


class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


def _args(**kw):
    return type("A", (ClipArgs,), kw)()


class _Dev:
    """Device state of one head: flat [W | b], its gradient and momentum, Pl."""

    def __init__(self, st, B, D, C):
        from mla_hip import ops
        f32 = dict(device="cuda", dtype=torch.float32)
        self.B, self.D, self.C, self.n = B, D, C, C * D
        self.flat, self.grad, self.buf = (torch.zeros(C * D + C, **f32) for _ in range(3))
        self.Pl = torch.empty((D, D), **f32)
        self.logits, self.loss, self.dX = torch.empty((B, C), **f32), torch.empty(1, **f32), torch.empty((B, D), **f32)
        self.r = torch.empty(D, **f32)
        self.ws = torch.empty(ops.feature_ws_elems(B, D, C), **f32)
        self.hws, self.gws = torch.empty(ops.head_ws_elems(B, C), **f32), torch.empty(ops.gs_ws_elems(D, C), **f32)
        self.load(st)

    W = property(lambda s: s.flat[:s.n].view(s.C, s.D))
    b = property(lambda s: s.flat[s.n:])

    def load(self, st):
        self.W.copy_(st.head["weight"])
        self.b.copy_(st.head["bias"])
        self.Pl.copy_(st.Pl)
        if st.mom["weight"] is not None:
            self.buf[:self.n].view(self.C, self.D).copy_(st.mom["weight"])
            self.buf[self.n:].copy_(st.mom["bias"])

    def fused(self, X, label, project, alpha, first):
        from mla_hip import ops
        ops.feature_phase(X, label, self.W, self.b, self.buf, self.Pl, self.logits, self.loss, self.ws, 1.0 / self.B, project, alpha,
                          LR, MOM, WD, first)

    def chain(self, X, label, project, alpha, first):
        """head_ce_fwd_bwd -> colsum -> gs_project -> sgd_step: what MLATrainer runs per phase for the other models."""
        from mla_hip import ops
        dW, db = self.grad[:self.n].view(self.C, self.D), self.grad[self.n:]
        ops.head_ce_fwd_bwd(X, self.W, self.b, label, self.logits, self.loss, dW, db, self.dX, self.hws, 1.0 / self.B)
        if project:
            ops.colsum(X, self.r, 1.0 / self.B)
            ops.gs_project(self.Pl, self.r, dW, alpha, self.gws)
        ops.sgd_step(self.flat, self.grad, self.buf, LR, MOM, WD, first)

    def outputs(self):
        return {"logits": self.logits.clone(), "loss": self.loss.clone(), "Pl": self.Pl.clone(), "W": self.W.clone(),
                "b": self.b.clone(), "buf": self.buf.clone()}


# ---- 1. phase vs chain and vs oracle -------------------------------------------------------------------------------------------------
# Seeds and features are chosen on the CPU alone: the comparison with the fp32 oracle at the tolerances above says something only
# where the oracle itself has that accuracy, so a case's seed is the first of 400 + B, 1400 + B, ... at which the oracle's own Pl
# (fp32 against the same phase in fp64 from the same state) stays within 1/16 of the tolerance in all three phases (here: 2 - 3 %;
# the test asserts 1/8, for CPUs that round differently).  Features are `.abs()` normals of mean 0.3, std 0.7 (the regime of
# gs_kat_d512).  At batch one no seed of that regime qualifies -- r is then one sample instead of a batch mean, k_i r_j spreads
# far enough to meet -alpha, and the fp32 oracle is 20 - 480 times outside the tolerance in the third phase -- so batch one draws
# |N(0.6, 0.06)|, the spread a 64-sample mean of the other cases' features has: it probes the B = 1 paths, not the conditioning.
PHASE_CASES = [(64, 512, 101, 464), (5, 768, 128, 3405), (1, 512, 3, 401), (8, 70, 65, 408), (3, 64, 64, 2403)]


def _phase_features(seed, ph, B, D, C):
    if B == 1:
        return O.portable_normal(seed + ph, (B, D), stream=21, mean=0.6, std=0.06).abs()
    return R.clip_inputs(seed, ph, B, D, C)[0].squeeze(1).contiguous()


@pytest.mark.parametrize("B,D,C,seed", PHASE_CASES)
def test_phase_vs_chain_and_oracle(B, D, C, seed):
    """Both halves of the two-slot softmax, the C = 128 limit, a D that is no multiple of 64 or 4, batch one.  Three consecutive
    phases from one state: first / not, project 0, 1, 1, alpha of batch_index 0, 1, 2 of 5.  Logits and loss of the fused call keep
    the chain's summation order: bit-equal as well as long as both sides hold the same head, i.e. in the first two phases (Pl and
    what follows a projected update are not: the fused projection is carried in fp64)."""
    st = R.ClipState(O.make_head_params(D, C, seed), D)
    fu, ch = _Dev(st, B, D, C), _Dev(st, B, D, C)
    n = C * D
    for ph in range(3):
        X = _phase_features(seed, ph, B, D, C)
        label = O.portable_labels(seed + ph, B, C)
        project, alpha, first = ph > 0, O.gs_alpha(ph, 5), ph == 0
        s64 = st.clone(torch.float64)
        R.gs_phase(s64, X.double(), label, ph, 5, LR, MOM, WD)
        ref = R.gs_phase(st, X, label, ph, 5, LR, MOM, WD)
        own = (st.Pl.double() - s64.Pl).abs().max().item()                      # the seed rule, checked where the test runs
        assert own <= (1e-8 + 2e-5 * s64.Pl.abs().max().item()) / 8, (ph, own)
        Xd, ld = X.cuda(), label.cuda()
        same_head = torch.equal(fu.flat, ch.flat)           # true until a projected update, which the two round differently
        assert same_head or ph == 2
        fu.fused(Xd, ld, project, alpha, first)
        ch.chain(Xd, ld, project, alpha, first)
        torch.cuda.synchronize()
        proj = dict(atol=1e-8, rtol=2e-5) if ph > 0 else dict(atol=1e-7, rtol=1e-6)     # from phase 1 on W carries projected updates
        for k in ("logits", "loss"):
            if same_head:
                assert torch.equal(getattr(fu, k), getattr(ch, k)), f"phase {ph}: fused {k} is not the chain's bit for bit"
            assert_close(getattr(fu, k), getattr(ch, k), atol=2e-6, rtol=2e-6, name=f"phase {ph} fused vs chain {k}")
        assert_close(fu.Pl, ch.Pl, atol=1e-8, rtol=2e-5, name=f"phase {ph} fused vs chain Pl")
        assert_close(fu.flat, ch.flat, name=f"phase {ph} fused vs chain parameters", **proj)
        assert_close(fu.buf, ch.buf, name=f"phase {ph} fused vs chain momentum", **proj)
        for name, dev in (("fused", fu), ("chain", ch)):
            tag = f"{name} phase {ph}"
            assert_close(dev.logits, ref["out"], atol=2e-6, rtol=2e-6, name=tag + " logits")
            assert_close(dev.loss.reshape(()), ref["loss"], atol=2e-6, rtol=2e-6, name=tag + " loss")
            assert_close(dev.Pl, st.Pl, atol=1e-8, rtol=2e-5, name=tag + " Pl")
            assert_close(dev.W, st.head["weight"], name=tag + " W", **proj)
            assert_close(dev.buf[:n].view(C, D), st.mom["weight"], name=tag + " momentum W", **proj)
            assert_close(dev.b, st.head["bias"], atol=1e-7, rtol=1e-6, name=tag + " b")
            assert_close(dev.buf[n:], st.mom["bias"], atol=1e-7, rtol=1e-6, name=tag + " momentum b")


# ---- 2. reproducible -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("project", [False, True])
def test_phase_is_reproducible(project):
    B, D, C, seed = 64, 512, 101, 17
    st = R.ClipState(O.make_head_params(D, C, seed), D)
    X = R.clip_inputs(seed, 0, B, D, C)[0].squeeze(1).contiguous()
    R.gs_phase(st, X, O.portable_labels(seed, B, C), 0, 5)                     # a state with momentum and, next, a non-trivial Pl
    R.gs_phase(st, X, O.portable_labels(seed, B, C), 1, 5)
    X, label = R.clip_inputs(seed, 1, B, D, C)[0].squeeze(1).contiguous().cuda(), O.portable_labels(seed + 1, B, C).cuda()
    outs = []
    for _ in range(2):
        dev = _Dev(st, B, D, C)
        dev.fused(X, label, project, O.gs_alpha(2, 5), False)
        torch.cuda.synchronize()
        outs.append(dev.outputs())
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(outs[0]["Pl"].cpu(), st.Pl) != project                  # Pl moves exactly when the projection fires


def test_bad_label_poisons_the_loss():
    B, D, C = 4, 64, 6
    st = R.ClipState(O.make_head_params(D, C, 3), D)
    dev = _Dev(st, B, D, C)
    X = R.clip_inputs(3, 0, B, D, C)[0].squeeze(1).contiguous().cuda()
    dev.fused(X, torch.tensor([0, 6, 1, 2], device="cuda"), False, 0.1, True)
    torch.cuda.synchronize()
    assert torch.isnan(dev.loss).all() and torch.isfinite(dev.logits).all()


# ---- 3. mixed-sign features, the same inputs on both sides ---------------------------------------------------------------------------
def _ulp32(x):
    import math
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23)


def test_mixed_sign_projection_error_vs_fp64():
    """The projection is ill-conditioned once features change sign: some of the D * D element-wise denominators alpha + k_i r_j come
    close to zero.  Teacher forcing: before each of three projecting phases the device gets the CPU fp32 oracle's state; the phase
    is also evaluated in fp64 on the CPU from that state.  The kernel's error against fp64 may be at most twice the fp32 oracle's,
    + 1e-7, in max-abs over Pl and over the projected update of W (and its momentum, which is that update without the factor lr).

    Seed, chosen on the CPU alone: over seeds 211 .. 230 the closest denominator of the second projecting phase lies 0 .. 115
    ulp(alpha) from zero (at 218 the fp32 oracle itself divides by zero and returns NaN, so there is nothing to compare with).  The
    seed is the one that keeps the fp32 oracle's denominators farthest from zero, 229 (115 ulp; the test asserts >= 32), so that the
    oracle's own error is finite and non-zero: 5.8e-10 / 5.3e-3 / 4.4e-4 on Pl over the three phases on one CPU.

    History of this check: with r, k and the denominator in fp32, as in the chain, the device's error is a random
    draw of the same size as the oracle's -- a CPU emulation of that arithmetic gives ratios between 0.02 and 5.8 over 14 such
    phases, and an MI355X gave 0.84 in phase 1 and 306 in phase 2 (7.2e-4 against an oracle that happened to land at 2.4e-6).  No
    summation order fixes that: one rounding of k_i r_j is worth 0.25 % of the dominant element at 395 ulp.  The fused phase therefore
    carries r, k, the denominator, the norm and the projected sums in fp64 and rounds each stored value once."""
    B, D, C, seed = 64, 512, 101, 229
    st = R.ClipState(O.make_head_params(D, C, seed + 2), D)
    st.exp_count = 1
    dev = _Dev(st, B, D, C)
    n = C * D
    for ph in range(3):
        X = R.clip_inputs(seed, ph, B, D, C, absolute=False)[0].squeeze(1).contiguous()
        label = O.portable_labels(seed + ph, B, C)
        assert (X < 0).any() and (X > 0).any()
        alpha = O.gs_alpha(ph, 5)
        r64 = X.double().mean(0, keepdim=True)
        den = (alpha + (st.Pl.double() @ r64.t()) @ r64).abs().min().item()
        assert den >= 32 * _ulp32(alpha), (ph, den / _ulp32(alpha))             # the seed rule, checked where the test runs
        s64, s32 = st.clone(torch.float64), st.clone()
        R.gs_phase(s64, X.double(), label, ph, 5, LR, MOM, WD)
        R.gs_phase(s32, X, label, ph, 5, LR, MOM, WD)
        dev.load(st)                                                            # teacher forcing
        W0 = st.head["weight"].double()
        dev.fused(X.cuda(), label.cuda(), True, alpha, st.mom["weight"] is None)
        torch.cuda.synchronize()
        got = {"Pl": dev.Pl.cpu().double(), "dW": dev.W.cpu().double() - W0, "momentum": dev.buf[:n].view(C, D).cpu().double()}
        o32 = {"Pl": s32.Pl.double(), "dW": s32.head["weight"].double() - W0, "momentum": s32.mom["weight"].double()}
        o64 = {"Pl": s64.Pl, "dW": s64.head["weight"] - W0, "momentum": s64.mom["weight"]}
        errs = {k: ((got[k] - o64[k]).abs().max().item(), (o32[k] - o64[k]).abs().max().item()) for k in got}
        for k, (e_hip, e_orc) in errs.items():
            print(f"phase {ph} {k}: min|den| {den / _ulp32(alpha):.0f} ulp, err(HIP, fp64) = {e_hip:.3e}, err(oracle fp32, fp64) = "
                  f"{e_orc:.3e}, ratio {e_hip / max(e_orc, 1e-300):.3f}")
        for k, (e_hip, e_orc) in errs.items():
            assert 0.0 < e_orc < float("inf"), (ph, k, e_orc)
            assert e_hip <= 2.0 * e_orc + 1e-7, (ph, k, e_hip, e_orc)
        st = s32


# ---- trainers -------------------------------------------------------------------------------------------------------------------------
def _trainer(seed, D=512, C=101, dataset="Food101", gs_mode="as_intended", lr=LR, **kw):
    from mla_hip import CLIPClassifier, MLATrainer
    model = CLIPClassifier(_args(dataset=dataset), seed=0, feat_dim=D)
    hd = O.make_head_params(D, C, seed + 2)
    model.load_state_dict({f"fusion_module.fc_out.{k}": v for k, v in hd.items()})
    return model, MLATrainer(model, lr=lr, momentum=MOM, weight_decay=WD, gs_mode=gs_mode, **kw), hd


# ---- 4. step vs the reference fixture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag,gs_mode", [("intended", "as_intended"), ("published", "as_published")])
def test_step_vs_reference_fixture(tag, gs_mode, fused, golden_dir):
    fx = np.load(os.path.join(golden_dir, "clip_small.npz"))
    B, D, C, steps, seed, ldl = [int(v) for v in fx["meta"]]
    model, tr, _ = _trainer(seed, D, C, gs_mode=gs_mode)
    tr.fused_feature_phase = fused
    assert not tr._estreams                                                     # no encoder streams for a feature-only model
    for s in range(steps):
        tok, img, label = R.clip_inputs(seed, s, B, D, C)
        losses = tr.train_step(tok.cuda(), img.cuda(), label.cuda(), s, ldl)
        torch.cuda.synchronize()
        tol = TOL if s == 0 else 1e-3
        assert set(losses) == {"loss", "loss_a", "loss_v"}
        assert torch.equal(tr.last["a"].cpu(), tok.squeeze(1)) and torch.equal(tr.last["v"].cpu(), img.squeeze(1))
        for k in ("out_a", "out_v"):
            assert_close(tr.last[k], fx[f"{tag}.s{s}.{k}"], atol=tol, name=f"{tag} s{s} {k}")
        for k in ("loss", "loss_a", "loss_v"):
            assert_close(losses[k].reshape(()), fx[f"{tag}.s{s}.{k}"], atol=tol, name=f"{tag} s{s} {k}")
        Pl = tr.gs_plugin.Pl.cpu()
        assert_close(Pl[:8, :8], fx[f"{tag}.s{s}.Pl.corner"], atol=1e-6, rtol=1e-4, name="Pl corner")
        assert_close(Pl[::16, ::16], fx[f"{tag}.s{s}.Pl.sub"], atol=1e-6, rtol=1e-4, name="Pl sub")
        assert abs(torch.trace(Pl).item() - float(fx[f"{tag}.s{s}.Pl.trace"])) < 1e-4
        assert abs(torch.linalg.norm(Pl).item() - float(fx[f"{tag}.s{s}.Pl.fro"])) < 1e-4
    assert tr.gs_plugin.exp_count == 2 * steps
    sd = model.state_dict()
    n = C * D
    mw, mb = tr.optimizer.buf["head"][:n].view(C, D), tr.optimizer.buf["head"][n:]
    pick, sfx = ((lambda t: t), "") if tag == "intended" else ((lambda t: t[:, ::4]), ".col4")
    assert_close(pick(sd["fusion_module.fc_out.weight"]), fx[f"{tag}.head.weight{sfx}"], atol=1e-3, name="head weight")
    assert_close(sd["fusion_module.fc_out.bias"], fx[f"{tag}.head.bias"], atol=1e-3, name="head bias")
    assert_close(pick(mw), fx[f"{tag}.momentum.weight{sfx}"], atol=1e-3, name="weight momentum")
    assert_close(mb, fx[f"{tag}.momentum.bias"], atol=1e-3, name="bias momentum")


# ---- 5. fused vs fused_feature_phase = False ---------------------------------------------------------------------------------------------
# The two paths evaluate the projection in fp64 and in fp32, and four free-running steps (seven projecting phases) amplify that: the
# fp32 CPU restatement against the fp64 one ends 0.06 - 1.2 tolerances apart over seeds 29, 129, ...  The seed of a case is the
# first of that sequence at which it ends within 1/8 (CPU only; checked below at 1/4).
@pytest.mark.parametrize("D,C,dataset,seed", [(512, 101, "Food101", 1529), (768, 6, "CREMAD", 829)])
def test_fused_step_equals_chain_step(D, C, dataset, seed):
    B = 16
    s32 = R.ClipState(O.make_head_params(D, C, seed + 2), D)
    s64 = s32.clone(torch.float64)
    for s in range(4):
        tok, img, label = R.clip_inputs(seed, s, B, D, C)
        R.clip_gs_step(s32, tok, img, label, s, 5, LR, MOM, WD)
        R.clip_gs_step(s64, tok.double(), img.double(), label, s, 5, LR, MOM, WD)
    for got, want in ((s32.Pl, s64.Pl), (s32.head["weight"], s64.head["weight"]), (s32.mom["weight"], s64.mom["weight"])):
        assert (got.double() - want).abs().max().item() <= (1e-8 + 2e-5 * want.abs().max().item()) / 4
    runs = []
    for fused in (True, False):
        model, tr, _ = _trainer(seed, D, C, dataset)
        tr.fused_feature_phase = fused
        rec = []
        for s in range(4):
            tok, img, label = R.clip_inputs(seed, s, B, D, C)
            losses = tr.train_step(tok.cuda(), img.cuda(), label.cuda(), s, 5)
            rec.append({"out_a": tr.last["out_a"].clone(), "out_v": tr.last["out_v"].clone(),
                        **{k: v.clone() for k, v in losses.items()}})
        torch.cuda.synchronize()
        runs.append((model, tr, rec))
    (mf, tf, rf), (mc, tc, rc) = runs
    for s in range(4):
        for k in rf[s]:
            assert_close(rf[s][k], rc[s][k], atol=2e-6, rtol=2e-6, name=f"s{s} {k}")
    assert_close(tf.gs_plugin.Pl, tc.gs_plugin.Pl, atol=1e-8, rtol=2e-5, name="Pl")
    assert_close(mf.fusion_module.fc_out.flat, mc.fusion_module.fc_out.flat, atol=1e-8, rtol=2e-5, name="head")
    assert_close(tf.optimizer.buf["head"], tc.optimizer.buf["head"], atol=1e-8, rtol=2e-5, name="momentum")
    assert tf.gs_plugin.exp_count == tc.gs_plugin.exp_count == 8 and tf.optimizer.initialized["head"]
    # keep_debug and Adam take the chain (the hooks need the raw and the projected gradient in memory)
    model, tr, _ = _trainer(seed, D, C, dataset)
    tr.keep_debug = True
    tok, img, label = R.clip_inputs(seed, 0, B, D, C)
    tr.train_step(tok.cuda(), img.cuda(), label.cuda(), 0, 5)
    assert "head_grad_a_raw" in tr.last and "head_grad_v" in tr.last
    model, tr, _ = _trainer(seed, D, C, dataset, optimizer="adam")
    losses = tr.train_step(tok.cuda(), img.cuda(), label.cuda(), 0, 5)
    assert torch.isfinite(losses["loss"]).all() and tr.optimizer.steps["head"] == 2


# ---- 6. the reference's loop lines on the protocol objects ----------------------------------------------------------------------------
def test_reference_loop_verbatim():
    """main.py:428-454, 468-472 verbatim on CLIPClassifier / fc_out / CrossEntropyLoss / GSPlugin / FusedSGD against MLATrainer."""
    import mla_hip
    B, D, C, seed = 8, 512, 101, 47
    model, tr, hd = _trainer(seed, D, C)

    class args:
        lorb, modal3, clip = "base", False, True
    pm = mla_hip.CLIPClassifier(_args(), seed=0)
    pm.load_state_dict({f"fusion_module.fc_out.{k}": v for k, v in hd.items()})
    model_p = mla_hip.DataParallel(pm, device_ids=[0])
    optimizer = mla_hip.FusedSGD(model_p.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    gs_plugin = mla_hip.GSPlugin(mode="as_intended")
    criterion = mla_hip.CrossEntropyLoss()
    av_alpha, len_dataloader = 0.55, 5
    model_p.train()
    for batch_step in range(3):
        tok, img, label = (t.cuda() for t in R.clip_inputs(seed, batch_step, B, D, C))
        spec, image = tok, img
        model = model_p
        optimizer.zero_grad()
        if args.clip:
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
            if p.grad != None:      # noqa: E711
                del p.grad

        _loss = (loss_a * av_alpha + loss_v * (1 - av_alpha)).item()

        losses = tr.train_step(tok, img, label, batch_step, len_dataloader)
        torch.cuda.synchronize()
        assert_close(tr.last["out_a"], out_a.detach(), atol=2e-6, rtol=2e-6, name="out_a")
        assert_close(tr.last["out_v"], out_v.detach(), atol=2e-6, rtol=2e-6, name="out_v")
        assert_close(losses["loss_a"].reshape(()), loss_a.detach(), atol=2e-6, rtol=2e-6, name="loss_a")
        assert_close(losses["loss_v"].reshape(()), loss_v.detach(), atol=2e-6, rtol=2e-6, name="loss_v")
        assert abs(losses["loss"].item() - _loss) <= 2e-6 + 2e-6 * abs(_loss)
    assert gs_plugin.exp_count == tr.gs_plugin.exp_count == 6
    assert_close(tr.gs_plugin.Pl, gs_plugin.Pl, atol=1e-8, rtol=2e-5, name="Pl")
    assert_close(tr.model.fusion_module.fc_out.flat, pm.fusion_module.fc_out.flat, atol=1e-8, rtol=2e-5, name="head")


# ---- 7. joint ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,dataset", [(3, "MVSA"), (101, "Food101")])
def test_joint_trainer_vs_autograd(C, dataset):
    """gs_flag false: JointTrainer / JointEvaluator on the concatenated-head kernels, against plain torch autograd with
    torch.optim.SGD (tolerance of tests/test_joint_gpu.py's loop comparison: 1e-5).  OGM / OGM-GE only touch 4-D conv gradients
    (main.py:392-408); this model has none, so the parameters equal Normal's bit for bit."""
    from mla_hip import CLIPClassifier, JointEvaluator, JointTrainer
    B, D, seed = 8, 512, 61
    hd = O.make_head_params(2 * D, C, seed + 2)
    ref = R.JointRef(hd, LR, MOM, WD)
    trainers = {}
    for mod in ("Normal", "OGM_GE"):
        model = CLIPClassifier(_args(dataset=dataset, gs_flag=False, modulation=mod), seed=0)
        model.load_state_dict({f"fusion_module.fc_out.{k}": v for k, v in hd.items()})
        trainers[mod] = (model, JointTrainer(model, lr=LR, momentum=MOM, weight_decay=WD, modulation=mod))
    for s in range(2):
        tok, img, label = R.clip_inputs(seed, s, B, D, C)
        rec = ref.step(tok, img, label)
        for mod, (model, tr) in trainers.items():
            losses = tr.train_step(tok.cuda(), img.cuda(), label.cuda(), s)
            torch.cuda.synchronize()
            assert_close(tr.last["out"], rec["out"], atol=1e-5, name=f"{mod} s{s} out")
            assert_close(tr.last["out_m"][0], rec["out_a"], atol=1e-5, name=f"{mod} s{s} out_a")
            assert_close(tr.last["out_m"][1], rec["out_v"], atol=1e-5, name=f"{mod} s{s} out_v")
            for k in ("loss", "loss_a", "loss_v"):
                assert_close(losses[k].reshape(()), rec[k], atol=1e-5, name=f"{mod} s{s} {k}")
            sd = model.state_dict()
            assert_close(sd["fusion_module.fc_out.weight"], rec["weight"], atol=1e-5, name=f"{mod} s{s} weight")
            assert_close(sd["fusion_module.fc_out.bias"], rec["bias"], atol=1e-5, name=f"{mod} s{s} bias")
        assert trainers["OGM_GE"][1].last["coeff"].shape[0] >= 2               # the coefficients are still reported
    assert torch.equal(trainers["Normal"][0].fusion_module.fc_out.flat, trainers["OGM_GE"][0].fusion_module.fc_out.flat)
    # evaluator counts: arg-max of out / out_a / out_v per class
    model = trainers["Normal"][0]
    ev = JointEvaluator(model)
    tok, img, label = R.clip_inputs(seed, 9, 16, D, C)
    out, out_m = ev.update(tok.cuda(), img.cuda(), label.cuda())
    torch.cuda.synchronize()
    want = [(o.cpu().argmax(1) == label).sum().item() / 16 for o in (out, out_m[0], out_m[1])]
    assert ev.result() == tuple(want)
    W, b = model.fusion_module.fc_out.weight.detach().cpu(), model.fusion_module.fc_out.bias.detach().cpu()
    assert_close(out, R.clip_forward(tok, img, False, W, b)[2], atol=2e-5, name="eval out")
    a, v, o = model(tok.cuda(), img.cuda())                                    # forward: (a, v, out) with gs_flag false
    assert torch.equal(a.cpu(), tok.squeeze(1)) and torch.equal(o, out)


# ---- 8. evaluator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dynamic", [False, True])
def test_evaluator_vs_oracle(dynamic):
    from mla_hip import Evaluator
    B, D, C, seed = 16, 512, 6, 71
    model, _tr, hd = _trainer(seed, D, C, "CREMAD")
    ev = Evaluator(model, dynamic=dynamic, av_alpha=0.5)
    tok, img, label = R.clip_inputs(seed, 0, B, D, C)
    outs = ev.update(tok.cuda(), img.cuda(), label.cuda())
    torch.cuda.synchronize()
    ref_outs = [x.squeeze(1) @ hd["weight"].t() + hd["bias"] for x in (tok, img)]
    for o, r in zip(outs, ref_outs):
        assert_close(o, r, atol=2e-6, rtol=2e-6, name="eval logits")
    w_ref, c_ref = O.valid_batch([o.cpu() for o in outs], label, C, dynamic, [0.5, 0.5])
    assert_close(ev.weights[:2], torch.tensor(w_ref), atol=1e-5, name="fusion weights")
    assert (ev.counts.view(4, C).cpu() == c_ref.int()).all()


# ---- 9. batcher -------------------------------------------------------------------------------------------------------------------------
def _feature_dir(tmp_path, N, D, seed):
    rng = np.random.default_rng(seed)
    names = [f"img_{i:03d}" for i in range(N)]
    text, vis = tmp_path / "text", tmp_path / "visual"
    text.mkdir()
    vis.mkdir()
    for n in names:
        np.save(text / (n + ".npy"), rng.standard_normal((1, D)).astype(np.float32))
        np.save(vis / (n + ".npy"), rng.standard_normal((1, D)).astype(np.float32))
    return names, [int(v) for v in rng.integers(0, 6, N)], str(text), str(vis)


@pytest.mark.parametrize("D", [512, 70])
def test_batcher_equals_host_indexing(D, tmp_path):
    from mla_hip import CLIPFeatureBatcher, epoch_permutation, load_feature_tables
    N, B = 37, 8
    names, labels, text, vis = _feature_dir(tmp_path, N, D, D)
    tok, img = load_feature_tables(names, text, vis)
    lab = torch.tensor(labels)
    for shuffle in (False, True):
        bt = CLIPFeatureBatcher(names, labels, B, text, vis, shuffle=shuffle, seed=3)
        assert len(bt) == 5
        for epoch in (0, 2):
            bt.set_epoch(epoch)
            order = epoch_permutation(N, shuffle, 3, epoch)
            got = list(bt)
            torch.cuda.synchronize()
            assert len(got) == 5 and got[-1][0].shape == (N - 4 * B, 1, D)       # the last, ragged batch
            for k, (t, i, l, ix) in enumerate(got):
                ids = order[k * B:(k + 1) * B]
                assert t.is_cuda and t.dtype == i.dtype == torch.float32 and t.shape == i.shape == (len(ids), 1, D)
                assert ix.dtype == l.dtype == torch.int64 and ix.shape == (len(ids), 1) and l.shape == (len(ids),)
                assert torch.equal(ix.cpu().flatten(), ids) and torch.equal(l.cpu(), lab[ids])
                assert torch.equal(t.cpu().squeeze(1), tok[ids]) and torch.equal(i.cpu().squeeze(1), img[ids])
    assert len(list(CLIPFeatureBatcher(names, labels, B, text, vis, drop_last=True))) == 4
    # the kernel clamps an index it should never have been handed, and never reads out of bounds
    from mla_hip import ops
    idx = torch.tensor([-5, 0, N - 1, N + 100], device="cuda")
    o0, o1 = torch.empty((4, D), device="cuda"), torch.empty((4, D), device="cuda")
    ol, oi = torch.empty(4, dtype=torch.int64, device="cuda"), torch.empty((4, 1), dtype=torch.int64, device="cuda")
    ops.gather_rows2(bt.token, bt.visual, bt.labels, idx, o0, o1, ol, oi)
    assert oi.flatten().tolist() == [0, 0, N - 1, N - 1] and torch.equal(o0.cpu(), tok[[0, 0, N - 1, N - 1]])
    r0, r1, rl, ri = torch.ops.mla_hip.gather_rows2(bt.token, bt.visual, bt.labels, idx[1:3])
    assert torch.equal(r1.cpu(), img[[0, N - 1]]) and rl.tolist() == [labels[0], labels[N - 1]] and ri.shape == (2, 1)


def test_batcher_loop_runs_without_host_sync(tmp_path):
    from mla_hip import CLIPFeatureBatcher
    N, B, D, C = 40, 8, 512, 6
    names, labels, text, vis = _feature_dir(tmp_path, N, D, 1)
    bt = CLIPFeatureBatcher(names, labels, B, text, vis, shuffle=True, seed=1)
    model, tr, _ = _trainer(5, D, C, "CREMAD")
    bt.set_epoch(0)                                                             # the epoch's one upload
    warm = next(iter(bt))
    tr.train_step(warm[0], warm[1], warm[2], 0, len(bt))                        # buffers allocated, library loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                    # any synchronising call raises from here on
    try:
        for step, (tok, img, label, _idx) in enumerate(bt):
            losses = tr.train_step(tok, img, label, step, len(bt))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(losses["loss"].item())


# ---- 10. checkpoint ----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_is_bitwise():
    B, D, C, seed = 8, 512, 101, 83
    batches = [tuple(t.cuda() for t in R.clip_inputs(seed, s, B, D, C)) for s in range(4)]
    model, tr, _ = _trainer(seed, D, C)
    for s in range(2):
        tr.train_step(*batches[s], s, 5)
    ck = {"model": {k: v.clone() for k, v in model.state_dict().items()}, "optimizer": tr.optimizer.state_dict(),
          "Pl": tr.gs_plugin.Pl.clone(), "exp_count": tr.gs_plugin.exp_count}
    for s in range(2, 4):
        tr.train_step(*batches[s], s, 5)
    model2, tr2, _ = _trainer(seed + 1, D, C)
    model2.load_state_dict(ck["model"])
    tr2.optimizer.load_state_dict(ck["optimizer"])
    tr2.gs_plugin.Pl.copy_(ck["Pl"])
    tr2.gs_plugin.exp_count = ck["exp_count"]
    for s in range(2, 4):
        tr2.train_step(*batches[s], s, 5)
    torch.cuda.synchronize()
    assert torch.equal(model.fusion_module.fc_out.flat, model2.fusion_module.fc_out.flat)
    assert torch.equal(tr.optimizer.buf["head"], tr2.optimizer.buf["head"])
    assert torch.equal(tr.gs_plugin.Pl, tr2.gs_plugin.Pl) and tr2.gs_plugin.exp_count == 8
    assert torch.equal(tr.last["out_v"], tr2.last["out_v"])


# ---- 11. learns ---------------------------------------------------------------------------------------------------------------------------
def test_training_learns_separable_features():
    """Class means in a shared embedding space plus noise, as paired text / image features are: 60 steps at lr 1e-2 with the shipped
    defaults (fused phase, projection as_intended).  The CPU restatement on such data goes from 1.8 / 1.3 to 0.08 / 0.06."""
    from mla_hip import Evaluator
    B, D, C, steps = 32, 512, 6, 60
    model, tr, _ = _trainer(5, D, C, "CREMAD", lr=1e-2)
    g = torch.Generator(device="cuda").manual_seed(0)
    M = O.portable_normal(3, (C, D), stream=7).cuda()

    def batch(n):
        label = torch.randint(0, C, (n,), device="cuda", generator=g)
        tok = M[label] + 0.5 * torch.randn((n, D), device="cuda", generator=g)
        img = M[label] + 0.5 * torch.randn((n, D), device="cuda", generator=g)
        return tok.unsqueeze(1), img.unsqueeze(1), label
    hist = []
    for s in range(steps):
        losses = tr.train_step(*batch(B), s % 10, 10)
        hist.append(torch.stack([losses["loss_a"].reshape(()), losses["loss_v"].reshape(())]).clone())
    hist = torch.stack(hist).cpu()
    assert torch.isfinite(hist).all()
    head, tail = hist[0], hist[40:].median(0).values
    assert (head > 1.0).all(), head
    assert (tail < 0.5 * head).all(), (head, tail)
    assert tr.gs_plugin.exp_count == 2 * steps and not torch.equal(tr.gs_plugin.Pl.cpu(), torch.eye(D))
    ev = Evaluator(model, av_alpha=0.5)
    ev.update(*batch(256))
    assert ev.result()[0] > 0.9, ev.result()


# ---- 12. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mla_hip import CLIPClassifier, MLATrainer, ops
    from mla_hip._lib import MLAHipError
    B, D = 4, 512
    f32 = dict(device="cuda", dtype=torch.float32)
    X, lab = torch.zeros((B, D), **f32), torch.zeros(B, dtype=torch.int64, device="cuda")

    def phase(C, X=X):
        flat, buf = torch.zeros(C * D + C, **f32), torch.zeros(C * D + C, **f32)
        ops.feature_phase(X, lab, flat[:C * D].view(C, D), flat[C * D:], buf, torch.eye(D, **f32), torch.empty((B, C), **f32),
                          torch.empty(1, **f32), torch.empty(max(ops.feature_ws_elems(B, D, min(C, 128)), 1) + D, **f32), 1.0 / B, True, 0.1, LR, MOM, WD,
                          True)
    phase(128)
    with pytest.raises(MLAHipError, match="C <= 128"):
        phase(129)
    with pytest.raises(MLAHipError):
        phase(6, X.half())
    with pytest.raises(MLAHipError):
        phase(6, X.cpu())
    with pytest.raises(Exception):                                              # the registered op has no CPU implementation
        torch.ops.mla_hip.feature_phase(X.cpu(), lab.cpu(), torch.zeros(6, D), torch.zeros(6), torch.zeros(6 * D + 6), None, 0.25, False,
                                        0.1, LR, MOM, WD, True)
    model, tr, _ = _trainer(5)
    tok = torch.zeros((B, 1, D), **f32)
    for bad in (tok.half(), torch.zeros((B, 2, D), **f32), tok.cpu()):
        with pytest.raises(MLAHipError, match="float32"):
            tr.train_step(bad, tok, lab, 0, 5)
        with pytest.raises(MLAHipError, match="float32"):
            model(tok, bad)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        MLATrainer(model, comm=type("C", (), dict(world=2, active=True))())
    with pytest.raises(NotImplementedError, match="QMF"):
        CLIPClassifier(_args(modulation="QMF"))
    torch.cuda.synchronize()
