"""GPU: the scalar-denominator head projector (gs_mode="owm") -- mla_gs_project_owm (csrc/gs_owm.hip) and the fused
mla_feature_phase_owm (csrc/feature_step.hip) against the fp64 restatement in tests/owm_model.py, its properties on the device, every
door to it (ops, torch.ops, GSPlugin's protocol and trainer paths, MLATrainer on CLIPClassifier and AVClassifier).

Tolerance: Pl, G and what a projected gradient reaches within GS_RTOL = 2e-5 of max |want| (the project's GS tolerance,
tests/tail_model.py).  The fp32 restatement itself is at most 1.4e-6 away at (768, 101): 7 % of it.  Measured on an MI355X
(error / tolerance, the largest over each test's cases): dense 0.013, Pl r = k alpha / s 0.0125, the phases' Pl 0.0035 and momentum
0.033, W 0.49 (one rounding of W against a tolerance of one ulp), the projected AVClassifier head gradient 0.024; the fused phase
and the chain gave the same figures to every printed digit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from util import assert_close  # noqa: E402
import clip_model as R  # noqa: E402
import owm_model as M  # noqa: E402
import tail_model as T  # noqa: E402

NAN = float("nan")
LR, MOM, WD = 1e-3, 0.9, 1e-4


def dev(t):
    return torch.as_tensor(t).float().contiguous().cuda()


def _ws(ops, D, C):
    return torch.full((ops.gs_owm_ws_elems(D, C),), NAN, device="cuda")


def _within(name, got, want, scale=None):
    """|got - want| <= GS_RTOL * max |want| (or * scale); prints error / tolerance as test_gs_project_vs_fp64 does."""
    got, want = got.detach().cpu().double(), want.double()
    assert torch.isfinite(got).all(), f"{name}: not fully written"
    tol = M.GS_RTOL * (want.abs().max().item() if scale is None else scale)
    err = (got - want).abs().max().item()
    print(f"owm {name}: error / tolerance = {err / tol if tol else float(err > 0):.3g}")
    assert err <= tol, (name, err, tol)


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops
    return ops


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_r", [False, True])
def test_exact_case_bit_for_bit(ops, zero_r):
    """D = 64, Pl = I, integer G, r = 0.5 at three places, s = 1 in both calls: every product, quotient and sum is exact, so Pl and G
    equal the fp64 restatement bit for bit after each call.  r = 0: k = 0, Pl and G do not move."""
    Pl0, G0, rs = M.exact_inputs()
    want = M.exact_case(torch.float64, zero_r)
    Pl, G, ws = dev(Pl0), dev(G0), _ws(ops, M.EXACT_D, M.EXACT_C)
    for call, (r, (_where, alpha)) in enumerate(zip(rs, M.EXACT_CALLS)):
        ops.gs_project_owm(Pl, dev(torch.zeros_like(r) if zero_r else r), G, alpha, ws)
        torch.cuda.synchronize()
        wPl, wG, _s = want[call]
        assert torch.equal(Pl.cpu().double(), wPl), f"call {call}: Pl"
        assert torch.equal(G.cpu().double(), wG), f"call {call}: G"
        ws.fill_(NAN)
    if zero_r:
        assert torch.equal(Pl.cpu(), Pl0) and torch.equal(G.cpu(), G0)


# ---- 2. dense against fp64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", M.DENSE_ALPHAS)
@pytest.mark.parametrize("D,C", T.GS_CASES)
def test_dense_vs_fp64(ops, D, C, alpha):
    """Two consecutive calls (the second from a non-identity Pl) on tests/tail_model.gs_case's inputs; the workspace starts as NaN, so
    a class or row that is not written shows."""
    c = M.dense_case(D, C, alpha)
    Pl, G, ws = torch.eye(D, device="cuda"), dev(c.G), _ws(ops, D, C)
    for call in range(2):
        ops.gs_project_owm(Pl, dev(c.rs[call]), G, alpha, ws)
        torch.cuda.synchronize()
        wPl, wG = c.want[call]
        _within(f"D={D} C={C} alpha={alpha} call {call} Pl", Pl, wPl)
        _within(f"D={D} C={C} alpha={alpha} call {call} G", G, wG)
        ws.fill_(NAN)


# ---- 3. properties on the device ---------------------------------------------------------------------------------------------------------
def _free_run(ops, D, C, calls):
    """[(Pl_before, r, alpha, Pl_after)] (host copies) of free-running calls from the identity, and the final G."""
    Pl, G, ws = torch.eye(D, device="cuda"), dev(O.portable_normal(40 + D, (C, D), stream=5)), _ws(ops, D, C)
    out = []
    for call, r in enumerate(M.feature_means(D, calls, 900)):
        alpha = O.gs_alpha(call % 10, 10)
        before = Pl.cpu()
        ops.gs_project_owm(Pl, dev(r), G, alpha, ws)
        torch.cuda.synchronize()
        out.append((before, r, alpha, Pl.cpu()))
    return out, G.cpu()


@pytest.mark.parametrize("D", [70, 257])
def test_properties_on_the_device(ops, D):
    """12 free-running calls: Pl stays symmetric bit for bit (the element update is symmetric in (i, j)); Pl_new r = k alpha / s --
    Pl_new r is the difference of Pl r = k and k (r . k) / s, both of the size of k, so the error is held to GS_RTOL of max |k|;
    two runs from the same inputs give the same bits (one order per sum, no atomics)."""
    run, G = _free_run(ops, D, 3, 12)
    for call, (before, r, alpha, after) in enumerate(run):
        assert torch.equal(after, after.t()), f"call {call}: Pl is not symmetric"
        k = before.double() @ r.double()
        s = alpha + r.double() @ k
        assert s.item() >= alpha
        _within(f"D={D} call {call} Pl r", after.double() @ r.double(), k * alpha / s, scale=k.abs().max().item())
    run2, G2 = _free_run(ops, D, 3, 12)
    assert torch.equal(G, G2) and all(torch.equal(a[3], b[3]) for a, b in zip(run, run2))
    assert not torch.equal(run[-1][3], torch.eye(D))


# ---- 4. every door ------------------------------------------------------------------------------------------------------------------------
def test_torch_ops_protocol_and_trainer_paths_equal_the_op(ops):
    from mla_hip import GSPlugin, torch_ops  # noqa: F401
    B, D, C, bi, ldl = 5, 70, 6, 3, 10
    alpha = GSPlugin.alpha(bi, ldl)
    X = dev(O.portable_normal(11, (B, D), stream=21, mean=0.3, std=0.7))
    G0 = dev(O.portable_normal(11, (C, D), stream=22))
    Pl0 = torch.eye(D, device="cuda")
    ops.gs_project_owm(Pl0, dev(O.portable_normal(11, (D,), stream=23)), G0.clone(), 0.1, _ws(ops, D, C))      # a non-identity start
    r = torch.empty(D, device="cuda")
    ops.colsum(X, r, 1.0 / B)
    wPl, wG = Pl0.clone(), G0.clone()
    ops.gs_project_owm(wPl, r, wG, alpha, _ws(ops, D, C))
    # torch.ops
    Pl, G = Pl0.clone(), G0.clone()
    torch.ops.mla_hip.gs_project_owm(Pl, X, G, alpha)
    assert torch.equal(Pl, wPl) and torch.equal(G, wG)
    # the protocol path: the gradient is read from and written through the head's weight.grad
    head = torch.nn.Linear(D, C, device="cuda")
    head.weight.grad = G0.clone()
    gs = GSPlugin(dim=D, device="cuda", mode="owm")
    gs.before_update(head, X, bi, ldl, 0)                                     # exp_count == 0 fires nothing
    assert torch.equal(gs.Pl, torch.eye(D, device="cuda")) and torch.equal(head.weight.grad, G0) and not gs._fired
    gs.Pl.copy_(Pl0)
    gs.before_update(head, X, bi, ldl, 1)
    assert torch.equal(gs.Pl, wPl) and torch.equal(head.weight.grad, wG) and gs._fired
    # the trainer path: a pre-reduced feature mean and the flat gradient view
    gs = GSPlugin(dim=D, device="cuda", mode="owm")
    gs.Pl.copy_(Pl0)
    G = G0.clone()
    gs.before_update(None, None, bi, ldl, 0, r_mean=r, grad=G)
    assert torch.equal(G, G0)
    gs.before_update(None, None, bi, ldl, 2, r_mean=r, grad=G)
    torch.cuda.synchronize()
    assert torch.equal(gs.Pl, wPl) and torch.equal(G, wG)
    # the literal mode on the same inputs is another rule
    gs = GSPlugin(dim=D, device="cuda", mode="as_intended")
    gs.Pl.copy_(Pl0)
    G = G0.clone()
    gs.before_update(None, None, bi, ldl, 2, r_mean=r, grad=G)
    assert not torch.equal(gs.Pl, wPl)


# ---- 5. the fused phase -------------------------------------------------------------------------------------------------------------------
class _Head:
    """Device state of one head: flat [W | b], its gradient and momentum, Pl."""

    def __init__(self, st, B, D, C, ops):
        f32 = dict(device="cuda", dtype=torch.float32)
        self.ops, self.B, self.D, self.C, self.n = ops, B, D, C, C * D
        self.flat, self.grad, self.buf = (torch.zeros(C * D + C, **f32) for _ in range(3))
        self.Pl = st.Pl.float().cuda()
        self.logits, self.loss, self.dX = torch.empty((B, C), **f32), torch.empty(1, **f32), torch.empty((B, D), **f32)
        self.r = torch.empty(D, **f32)
        self.ws = torch.full((ops.feature_ws_elems(B, D, C),), NAN, **f32)
        self.hws, self.gws = torch.empty(ops.head_ws_elems(B, C), **f32), torch.full((ops.gs_owm_ws_elems(D, C),), NAN, **f32)
        self.W.copy_(st.head["weight"])
        self.b.copy_(st.head["bias"])

    W = property(lambda s: s.flat[:s.n].view(s.C, s.D))
    b = property(lambda s: s.flat[s.n:])

    def fused(self, X, label, alpha, first):
        self.ops.feature_phase(X, label, self.W, self.b, self.buf, self.Pl, self.logits, self.loss, self.ws, 1.0 / self.B, True, alpha,
                               LR, MOM, WD, first, owm=True)

    def chain(self, X, label, alpha, first):
        """head_ce_fwd_bwd -> colsum -> gs_project_owm -> sgd_step: what MLATrainer runs per phase outside the fused path."""
        ops = self.ops
        dW, db = self.grad[:self.n].view(self.C, self.D), self.grad[self.n:]
        ops.head_ce_fwd_bwd(X, self.W, self.b, label, self.logits, self.loss, dW, db, self.dX, self.hws, 1.0 / self.B)
        ops.colsum(X, self.r, 1.0 / self.B)
        ops.gs_project_owm(self.Pl, self.r, dW, alpha, self.gws)
        ops.sgd_step(self.flat, self.grad, self.buf, LR, MOM, WD, first)

    def state64(self, exp_count):
        """The device's state as an fp64 ClipState: the next phase's reference starts where the device does."""
        st = R.ClipState.__new__(R.ClipState)
        st.head = {"weight": self.W.cpu().double(), "bias": self.b.cpu().double()}
        st.mom = {"weight": self.buf[:self.n].view(self.C, self.D).cpu().double(), "bias": self.buf[self.n:].cpu().double()}
        st.Pl, st.exp_count = self.Pl.cpu().double(), exp_count
        return st


PHASE_SHAPES = [(1, 64, 1), (5, 70, 6), (64, 257, 101), (65, 64, 128)]


@pytest.mark.parametrize("path", ["fused", "chain"])
@pytest.mark.parametrize("B,D,C", PHASE_SHAPES)
def test_phase_vs_fp64(ops, B, D, C, path):
    """Two projecting phases on mixed-sign features (the second starts from a non-identity Pl), each against the fp64 phase from the
    state the device starts it from: logits and loss as tests/test_clip_gpu.py holds them (2e-6 + 2e-6 rel), bias and its momentum
    likewise (1e-7 + 1e-6 rel), Pl and the weight's momentum within GS_RTOL of max |want|, W within lr times the momentum's
    tolerance plus one ulp of max |W| (W = W - lr * momentum, rounded once)."""
    seed = 700 + B + D + C
    hd = {k: v.double() for k, v in O.make_head_params(D, C, seed).items()}
    s64 = R.ClipState(hd, D)
    s64.exp_count = 1                                                        # the projection fires from the first phase of this test
    h = _Head(s64, B, D, C, ops)
    n = C * D
    for ph in range(2):
        X = R.clip_inputs(seed, ph, B, D, C, absolute=False)[0].squeeze(1).contiguous()
        label = O.portable_labels(seed + ph, B, C)
        ref = M.owm_phase(s64, X.double(), label, ph, 5, LR, MOM, WD)
        getattr(h, path)(X.cuda(), label.cuda(), O.gs_alpha(ph, 5), ph == 0)
        torch.cuda.synchronize()
        tag = f"{path} B={B} D={D} C={C} phase {ph}"
        assert_close(h.logits, ref["out"], atol=2e-6, rtol=2e-6, name=tag + " logits")
        assert_close(h.loss.reshape(()), ref["loss"], atol=2e-6, rtol=2e-6, name=tag + " loss")
        assert_close(h.b, s64.head["bias"], atol=1e-7, rtol=1e-6, name=tag + " b")
        assert_close(h.buf[n:], s64.mom["bias"], atol=1e-7, rtol=1e-6, name=tag + " momentum b")
        _within(tag + " Pl", h.Pl, s64.Pl)
        _within(tag + " momentum W", h.buf[:n].view(C, D), s64.mom["weight"])
        wW = s64.head["weight"]
        tolW = LR * M.GS_RTOL * s64.mom["weight"].abs().max().item() + float(np.spacing(np.float32(wW.abs().max().item())))
        errW = (h.W.cpu().double() - wW).abs().max().item()
        print(f"owm {tag} W: error / tolerance = {errW / tolW:.3g}")
        assert errW <= tolW, (tag, errW, tolW)
        assert not torch.equal(h.Pl.cpu(), torch.eye(D))
        assert torch.equal(h.Pl, h.Pl.t())                                   # symmetric bit for bit on this path too
        s64 = h.state64(s64.exp_count)


class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


def _clip_trainer(seed, D, C, **kw):
    from mla_hip import CLIPClassifier, MLATrainer
    model = CLIPClassifier(ClipArgs(), seed=0, feat_dim=D)
    hd = O.make_head_params(D, C, seed + 2)
    model.load_state_dict({f"fusion_module.fc_out.{k}": v for k, v in hd.items()})
    return model, MLATrainer(model, lr=LR, momentum=MOM, weight_decay=WD, gs_mode="owm", **kw), hd


def test_clip_trainer_fused_chain_restatement_and_resume():
    """Four steps of MLATrainer(CLIPClassifier, gs_mode="owm"): the fused phase and the chain against the fp64 restatement of the same
    four steps, and a run resumed after two steps from the saved head, momentum, Pl and exp_count ends bit-identical."""
    B, D, C, seed = 8, 512, 101, 83
    host = [R.clip_inputs(seed, s, B, D, C, absolute=False) for s in range(4)]
    batches = [tuple(t.cuda() for t in b) for b in host]
    s64 = R.ClipState({k: v.double() for k, v in O.make_head_params(D, C, seed + 2).items()}, D)
    for s, (tok, img, label) in enumerate(host):
        for feat in (tok, img):
            M.owm_phase(s64, feat.squeeze(1).double(), label, s, 5, LR, MOM, WD)
    want_flat = torch.cat([s64.head["weight"].reshape(-1), s64.head["bias"]])
    want_buf = torch.cat([s64.mom["weight"].reshape(-1), s64.mom["bias"]])
    for fused in (True, False):
        model, tr, _ = _clip_trainer(seed, D, C)
        tr.fused_feature_phase = fused
        assert tr._fused_ok() == fused
        for s in range(2):
            tr.train_step(*batches[s], s, 5)
        ck = {"model": {k: v.clone() for k, v in model.state_dict().items()}, "optimizer": tr.optimizer.state_dict(),
              "Pl": tr.gs_plugin.Pl.clone(), "exp_count": tr.gs_plugin.exp_count}
        for s in range(2, 4):
            tr.train_step(*batches[s], s, 5)
        torch.cuda.synchronize()
        tag = "fused" if fused else "chain"
        assert tr.gs_plugin.exp_count == 8 and tr.gs_plugin._fired
        _within(tag + " Pl after 4 steps", tr.gs_plugin.Pl, s64.Pl)
        _within(tag + " momentum after 4 steps", tr.optimizer.buf["head"], want_buf)
        assert_close(model.fusion_module.fc_out.flat, want_flat, atol=1e-7, rtol=1e-6, name=tag + " head")
        assert torch.equal(tr.gs_plugin.Pl, tr.gs_plugin.Pl.t())
        model2, tr2, _ = _clip_trainer(seed + 1, D, C)
        tr2.fused_feature_phase = fused
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
    # Adam takes the chain and projects with the same rule
    model, tr, _ = _clip_trainer(seed, D, C, optimizer="adam")
    for s in range(2):
        losses = tr.train_step(*batches[s], s, 5)
    torch.cuda.synchronize()
    assert torch.isfinite(losses["loss"]).all() and tr.optimizer.steps["head"] == 4
    assert not torch.equal(tr.gs_plugin.Pl, torch.eye(D, device="cuda")) and torch.equal(tr.gs_plugin.Pl, tr.gs_plugin.Pl.t())


# ---- 6. the trainer on encoders -----------------------------------------------------------------------------------------------------------
class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", True, "Normal"
    lorb, clip, modal3 = "base", False, False


def test_av_trainer_projects_with_the_rule():
    """Two train_steps of a small AVClassifier batch (the shapes of tests/test_protocol_gpu.py) with gs_mode="owm" and keep_debug: the
    head gradient after the projection is the restatement's on what went in (the raw gradient, Pl before, the features), phase by
    phase; the first phase of the run is skipped; exp_count counts four."""
    import mla_hip
    seed, B = 53, 4
    model = mla_hip.AVClassifier(AVArgs(), device="cuda:0", seed=0)
    sd = {f"audio_net.{k}": v for k, v in O.make_resnet18_params("audio", seed).items()}
    sd.update({f"visual_net.{k}": v for k, v in O.make_resnet18_params("visual", seed + 1).items()})
    sd.update({f"fusion_module.fc_out.{k}": v for k, v in O.make_head_params(512, 6, seed + 2).items()})
    model.load_state_dict(sd)
    tr = mla_hip.MLATrainer(model, lr=LR, momentum=MOM, weight_decay=WD, gs_mode="owm")
    tr.keep_debug = True
    fired = 0
    for step in range(2):
        spec = O.portable_normal(seed + 100 + step, (B, 128, 64), stream=1, mean=-5.081, std=4.4849).cuda()
        image = O.portable_normal(seed + 100 + step, (B, 3, 2, 64, 64), stream=2).cuda()
        label = O.portable_labels(seed + 100 + step, B, 6).cuda()
        losses = tr.train_step(spec, image, label, step, 10)
        tr.join()
        torch.cuda.synchronize()
        assert torch.isfinite(losses["loss"]).all()
        for ph, name in enumerate(("a", "v")):
            raw, got, before = (tr.last[f"head_grad_{name}_raw"], tr.last[f"head_grad_{name}"], tr.last[f"Pl_before_{name}"])
            if step == 0 and ph == 0:
                assert torch.equal(raw, got) and torch.equal(before, torch.eye(512, device="cuda"))
                continue
            feat = tr.last[name].cpu().double()
            assert feat.shape == (B, 512)
            wPl, wG, _k, _s = M.owm_ref(before.cpu(), feat.mean(dim=0), raw.cpu(), O.gs_alpha(step, 10))
            _within(f"AV step {step} phase {name} projected head gradient", got, wG)
            fired += 1
            if ph == 1:
                _within(f"AV step {step} Pl", tr.gs_plugin.Pl, wPl)
    assert fired == 3 and tr.gs_plugin.exp_count == 4 and tr.gs_plugin.mode == "owm"
    assert torch.equal(tr.gs_plugin.Pl, tr.gs_plugin.Pl.t())
