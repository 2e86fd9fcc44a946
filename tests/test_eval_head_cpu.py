"""CPU: the per-sample evaluation rule (tests/eval_model.py) against the reference's own expressions applied to one row, the
conditions the GPU tests of mla_eval_head rest on, the additive ABI entry's refusals (nothing is dereferenced before validation) and
Evaluator's argument rules."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_model as E
import tail_model as T
from oracle import mla_oracle as O

F32, F64 = np.float32, np.float64


class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,C", E.SAMPLE_DENSE)
def test_restatement_is_the_reference_rule_on_one_row(M, B, C):
    """On a 1-D tensor softmax(dim=0) is the sample's class distribution, so main.py:65-87 (oracle.gating_weights, and the
    same expressions written out here) applied to row r is the per-sample rule."""
    outs, label = E.sample_dense_case(M, B, C)
    m = E.eval_rows(outs, label, 1, T.EVAL_ALPHAS[M])
    worst = 0.0
    for r in range(B):
        rows = [torch.from_numpy(o[r]).double() for o in outs]
        ent = []
        for row in rows:
            p = F.softmax(row, dim=0)
            ent.append(-torch.sum(p * torch.log(p)))
        g = [torch.exp(max(ent) - e) for e in ent]
        want = np.array([float(x / sum(g)) for x in g])
        oracle = np.array([float(x) for x in O.gating_weights(rows)])
        assert np.abs(want - oracle).max() <= 1e-15
        worst = max(worst, float(np.abs(m.weights[r] - want).max()))
        fused = sum(w * row for w, row in zip(want, rows)).numpy()
        assert np.abs(m.fused[r] - fused).max() <= 1e-12
        assert m.pred[r, 0] == int(np.argmax(fused)) and list(m.pred[r, 1:]) == [int(row.argmax()) for row in rows]
    print(f"restatement vs the reference's expressions M={M} B={B} C={C}: weights off by {worst:.3g}")
    assert worst <= 1e-12
    # counters: rebuilt from the predictions; the per-modality ones are tail_model's (they do not depend on the weights)
    assert (m.counts[2:] == T.eval_counts(outs, label, T.EVAL_ALPHAS[M])[2:]).all()
    want_counts = np.zeros_like(m.counts)
    for r in range(B):
        want_counts[0, label[r]] += 1
        for k in range(1 + M):
            want_counts[1 + k, label[r]] += int(m.pred[r, k] == label[r])
    assert (m.counts == want_counts).all() and m.counts[0].sum() == B and not m.bad.any()


@pytest.mark.parametrize("M,B,C", E.SAMPLE_DENSE)
def test_dense_cases_meet_the_margin_and_fp32_stays_inside_the_tolerances(M, B, C):
    """The precondition of the GPU test, for exactly its seeds: every row's fp64 fused top-2 margin is at least EVAL_MARGIN, and
    an fp32 evaluation of the rule stays within the weight / fused tolerances and flips no arg-max."""
    outs, label = E.sample_dense_case(M, B, C)
    m64 = E.eval_rows(outs, label, 1, T.EVAL_ALPHAS[M])
    m32 = E.eval_rows(outs, label, 1, T.EVAL_ALPHAS[M], dtype=F32)
    margin = E.top2_margin(m64.fused)
    dw = float(np.abs(m32.weights.astype(F64) - m64.weights).max())
    df = float(np.abs(m32.fused.astype(F64) - m64.fused).max())
    print(f"dense M={M} B={B} C={C}: margin {margin:.3g}, fp32 weights off by {dw:.3g}, fused off by {df:.3g}")
    assert margin >= E.EVAL_MARGIN
    assert dw <= E.WEIGHT_TOL / 10 and df <= E.fused_tol(M, outs) / 2
    assert (m32.pred == m64.pred).all() and (m32.counts == m64.counts).all()
    assert np.abs(m64.weights.sum(axis=1) - 1).max() <= 1e-12


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("C", [2, 6, 65, 101, 128])
def test_equal_logits_give_every_modality_the_same_weight(M, C):
    row = O.portable_normal(C, (C,), stream=64).numpy()
    for dtype in (F64, F32):
        w = E.row_weights([row] * M, 1, None, [True] * M, dtype)
        assert (w == w[0]).all() and abs(float(w[0]) - 1.0 / M) <= 1e-7


@pytest.mark.parametrize("C", [2, 6, 65, 101, 128])
def test_saturated_modality_has_entropy_exactly_zero_in_fp32(C):
    """exp(-200) underflows to exactly 0 in fp32: those classes contribute 0 (the limit, not 0 * -inf), the peak contributes
    1 * log 1 = 0.  Against two uniform modalities (entropy log C) the saturated one gets C / (C + 2)."""
    assert np.exp(F32(-E.SATURATED)) == 0
    sat = E.saturated_row(C, C - 1)
    h = E.row_entropy(sat, F32)
    assert h == 0 and not np.isnan(h)
    uni = np.zeros(C, dtype=F32)
    assert abs(float(E.row_entropy(uni, F32)) - np.log(C)) <= 4 * np.spacing(F32(np.log(C)))
    w = E.row_weights([uni, sat, uni], 1, None, [True] * 3, F32)
    assert np.abs(w.astype(F64) - np.array([1, C, 1]) / (C + 2)).max() <= E.WEIGHT_TOL


def test_presence_rules_of_the_restatement():
    C, al = 6, (0.35, 0.25, 0.4)
    rows = [O.portable_normal(70 + m, (C,), stream=65, std=1.5).numpy() for m in range(3)]
    for pat in E.every_pattern(7):
        el = pat != 0
        for mode in (0, 1):
            w = E.row_weights(rows, mode, al, el)
            assert (w[~el] == 0).all() and not np.signbit(w[~el]).any() and abs(w.sum() - 1) <= 1e-12
        w0 = E.row_weights(rows, 0, al, el)
        assert np.abs(w0[el] - np.array(al)[el] / np.array(al)[el].sum()).max() <= 1e-15
        if el.sum() == 1:
            assert (E.row_weights(rows, 1, al, el)[el] == 1).all()
    # the gating over the eligible ones is the gating of those modalities alone
    w = E.row_weights(rows, 1, al, [True, False, True])
    assert np.abs(w[[0, 2]] - E.row_weights([rows[0], rows[2]], 1, al, [True, True])).max() <= 1e-15
    # bad rows: a label outside [0, C), no modality at all
    outs = [np.stack([r, r, r]) for r in rows]
    m = E.eval_rows(outs, np.array([-1, 2, C]), 1, al, present=np.array([[1, 1, 1], [0, 0, 0], [1, 1, 1]]))
    assert m.bad.all() and np.isnan(m.weights).all() and (m.pred == -1).all() and m.counts.sum() == 0
    # mode 0: the present modalities carry no share of the fusion (nothing to renormalise by); a full row keeps its alphas
    m = E.eval_rows(outs, np.array([1, 2, 3]), 0, (1.0, 0.0, 0.0), present=np.array([[0, 1, 1], [1, 0, 0], [1, 1, 1]]))
    assert m.bad.tolist() == [True, False, False] and (m.weights[1:] == [1, 0, 0]).all()
    assert not E.eval_rows(outs, np.array([1, 2, 3]), 1, (1.0, 0.0, 0.0), present=np.array([[0, 1, 1], [1, 0, 0], [1, 1, 1]])).bad.any()


def test_identity_head_hands_the_logits_through():
    W, b = E.identity_head(5)
    x = O.portable_normal(3, (4, 5), stream=66).numpy()
    assert (x @ W.T + b == x).all() and W.dtype == F32 and b.dtype == F32


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_abi_entry_is_additive_and_refuses_before_any_launch():
    from mla_hip import _lib, torch_ops
    lib = _lib.load()
    assert hasattr(lib, "mla_eval_head") and len(_lib.PROTOTYPES["mla_eval_head"][1]) == 21
    assert lib.mla_abi_version() == 3                        # additive
    assert "eval_head" in torch_ops.op_names()
    fake = 0x1000                                            # non-null, aligned, never dereferenced: validation fails first

    def call(M=2, B=4, D=64, C=6, mode=1, x2=None, logits=fake, labels=fake, fused=None):
        return lib.mla_eval_head(fake, fake, x2, fake, fake, labels, None, fake, logits, fused, None, None, M, B, D, C, mode, 0.5, 0.5,
                                 0.0, None)
    assert call(C=129) == -1 and b"mla_eval_head: need 0 < C <= 128 (got 129)" in lib.mla_last_error()
    assert call(M=1) == -1 and b"need M = 2 or 3 (got 1)" in lib.mla_last_error()
    assert call(M=4) == -1
    assert call(mode=2) == -1 and b"need mode = 0" in lib.mla_last_error()
    assert call(logits=None) == -1 and b"null pointer" in lib.mla_last_error()
    assert call(M=3) == -1 and b"null pointer" in lib.mla_last_error()                 # three modalities need x2
    assert call(B=0) == -1 and b"B, D, C > 0" in lib.mla_last_error()
    assert call(labels=fake + 4) == -1 and b"8-byte" in lib.mla_last_error()
    assert call(fused=fake + 2) == -1 and b"4-byte" in lib.mla_last_error()
    with pytest.raises(Exception):                           # no CPU implementation: torch's "no kernel" error
        torch.ops.mla_hip.eval_head([torch.zeros(2, 4), torch.zeros(2, 4)], torch.zeros(3, 4), torch.zeros(3),
                                    torch.zeros(2, dtype=torch.int64), torch.zeros(12, dtype=torch.int32), 1, [0.5, 0.5], None)


# ---- Evaluator's argument rules ------------------------------------------------------------------------------------------------------
def test_evaluator_argument_validation():
    from mla_hip import CLIPClassifier, Evaluator
    from mla_hip._lib import MLAHipError
    from mla_hip import trainer
    model = CLIPClassifier(ClipArgs(), device="cpu", seed=0, feat_dim=64)
    params = inspect.signature(Evaluator.__init__).parameters
    assert params["dynamic_mode"].default == "batch" and params["gate_absent"].default is False and params["dynamic"].default is False
    for bad in ("row", "", "Sample", None):
        with pytest.raises(ValueError, match="dynamic_mode"):
            Evaluator(model, dynamic=True, dynamic_mode=bad)
    with pytest.raises(MLAHipError, match="gate_absent"):                      # CLIPClassifier's forward takes no present=
        Evaluator(model, gate_absent=True)
    ev = Evaluator(model, dynamic=True)
    assert not ev.per_sample and ev.dynamic_mode == "batch"
    assert Evaluator(model, dynamic=True, dynamic_mode="sample").per_sample
    assert not Evaluator(model, dynamic=False, dynamic_mode="sample").per_sample   # fixed alphas: one rule, the published chain
    assert not hasattr(ev, "sample_weights") and ev.weights.shape == (3,)
    assert ev.per_class().shape == (4, 6) and ev.per_class().sum() == 0 and ev.result() == (0.0, 0.0, 0.0)

    class Stub:                                                                 # what Evaluator asks of a model
        device = torch.device("cpu")
        fusion_module = model.fusion_module

        def mla_encoders(self):
            return [("v", "image", None), ("t", "text", None), ("a", "audio", None)]

        def forward_raw(self, *inputs, present=None):
            return inputs

        def eval(self):
            return self
    assert trainer.takes_present(Stub()) and not trainer.takes_present(model)
    assert Evaluator(Stub(), gate_absent=True).per_sample and Evaluator(Stub(), dynamic=True, dynamic_mode="sample", gate_absent=True).per_sample
    with pytest.raises(ValueError, match="dynamic_mode='sample'"):
        Evaluator(Stub(), dynamic=True, gate_absent=True)
    # columns (audio, image, text) of the user's matrix land on the encoders by tag
    present = torch.tensor([[1, 0, 0], [0, 1, 1]], dtype=torch.uint8)
    got = trainer.present_in_encoder_order(Stub(), present, 2)
    assert got.dtype == torch.uint8 and got.tolist() == [[0, 0, 1], [1, 1, 0]]
    with pytest.raises(MLAHipError, match="no modality left"):
        trainer.present_in_encoder_order(Stub(), torch.zeros((2, 3), dtype=torch.uint8), 2)
