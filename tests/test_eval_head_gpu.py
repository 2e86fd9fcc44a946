"""mla_eval_head (csrc/eval_head.hip): features to counters in one launch with per-sample fusion weights, against the fp64 restatement
of tests/eval_model.py, against the kernels it fuses (head_logits, eval_fuse) and through Evaluator.

  exact (bit for bit)   logits_out vs ops.head_logits; counters and arg-maxes everywhere; the fixed-weight path on integer logits with
                        forced ties vs ops.eval_fuse; equal / permuted modalities; every float under a change of the batch split
  derived bound         weights 1e-5 (the project's tolerance on fusion weights); fused logits M * 1e-5 * max |logit|, the weight
                        tolerance carried through the sum; each row's weights sum to 1 within 1e-6

Every output starts filled (a NaN no kernel produces; -7 for integers) inside guarded buffers: each call must write all of it and
nothing else.  tests/test_eval_head_cpu.py proves the margins these bounds rest on.  Logits reach the kernel through the identity head
(W = I, b = 0: every dot has one non-zero term) wherever a test designs the logits themselves."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_model as E  # noqa: E402
import tail_model as T  # noqa: E402
from oracle import mla_oracle as O  # noqa: E402

F32, F64 = np.float32, np.float64
FILL = 0x7FC0BEEF          # a quiet NaN no kernel produces
IFILL = -7
GUARD = 256
ALPHAS3 = (0.35, 0.25, 0.4)          # main.py:488 defaults


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(device="cuda", dtype=dtype).contiguous()


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


def same_bits(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == F32 and want.dtype == F32 and got.shape == want.shape, f"{name}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{name}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


class Arena:
    """Guarded, filled device buffers of one call: fp32 (NaN pattern) and int32 (-7)."""

    def __init__(self):
        self.bufs = []

    def _new(self, shape, fill, name, as_float):
        n = math.prod(shape)
        flat = torch.full((n + 2 * GUARD,), fill, dtype=torch.int32, device="cuda")
        self.bufs.append((flat, n, fill, name))
        body = flat[GUARD:GUARD + n]
        return (body.view(torch.float32) if as_float else body).view(shape)

    def f32(self, *shape, name="out"):
        return self._new(shape, FILL, name, True)

    def i32(self, *shape, name="out"):
        return self._new(shape, IFILL, name, False)

    def check(self, written=True):
        """written: every element was written and the guards are intact; not written: nothing changed at all."""
        torch.cuda.synchronize()
        for flat, n, fill, name in self.bufs:
            assert bool((flat[:GUARD] == fill).all()) and bool((flat[GUARD + n:] == fill).all()), f"{name}: a guard was overwritten"
            left = int((flat[GUARD:GUARD + n] == fill).sum())
            assert left == (0 if written else n), f"{name}: {left} of {n} elements hold the fill"


def run_head(ops, feats, W, b, label, mode, alphas, present=None, counts=None, calls=1):
    """One (or `calls`) ops.eval_head call(s) on guarded outputs -> numpy views of everything it wrote; counts (2 + M, C)."""
    M, (B, _D), C = len(feats), feats[0].shape, W.shape[0]
    ar = Arena()
    logits, fused, weights = ar.f32(M, B, C, name="logits_out"), ar.f32(B, C, name="fused_out"), ar.f32(B, M, name="weights_out")
    pred = ar.i32(B, 1 + M, name="pred_out")
    if counts is None:
        counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    x, Wd, bd, lab = [dev(f) for f in feats], dev(W), dev(b), dev(label, torch.int64)
    pres = None if present is None else dev(np.asarray(present, dtype=np.uint8))
    for _ in range(calls):
        ops.eval_head(x, Wd, bd, lab, counts, logits, mode=mode, alphas=list(alphas), present=pres, fused_out=fused, weights_out=weights,
                      pred_out=pred)
    ar.check()
    return SimpleNamespace(logits=logits.cpu().numpy(), fused=fused.cpu().numpy(), weights=weights.cpu().numpy(),
                           pred=pred.cpu().numpy().astype(np.int64), counts=counts.view(2 + M, C).cpu().numpy().astype(np.int64),
                           logits_dev=logits, counts_dev=counts)


def through_identity(ops, outs, label, mode, alphas, **kw):
    W, b = E.identity_head(outs[0].shape[1])
    got = run_head(ops, outs, W, b, label, mode, alphas, **kw)
    for m, o in enumerate(outs):
        same_bits(got.logits[m], o, f"identity head: logits_out[{m}]")
    return got


def check_against_model(got, m, M, outs, name):
    """The tolerances of the dense sample-mode test: weights 1e-5, fused M * 1e-5 * max |logit|, counters and arg-maxes exact, each
    good row's weights summing to 1 within 1e-6; bad rows NaN / -1."""
    ok = ~m.bad
    dw = float(np.abs(got.weights[ok].astype(F64) - m.weights[ok]).max()) if ok.any() else 0.0
    df = float(np.abs(got.fused[ok].astype(F64) - m.fused[ok]).max()) if ok.any() else 0.0
    ds = float(np.abs(got.weights[ok].astype(F64).sum(axis=1) - 1).max()) if ok.any() else 0.0
    print(f"{name}: weights off by {dw:.3g} (tol {E.WEIGHT_TOL:g}), fused off by {df:.3g} (tol {E.fused_tol(M, outs):.3g}), row sums off by {ds:.3g}")
    assert dw <= E.WEIGHT_TOL and df <= E.fused_tol(M, outs) and ds <= 1e-6
    assert (got.pred == m.pred).all(), np.argwhere(got.pred != m.pred)[:5]
    assert (got.counts == m.counts).all(), (got.counts, m.counts)
    assert np.isnan(got.weights[m.bad]).all() and np.isnan(got.fused[m.bad]).all() and (got.pred[m.bad] == -1).all()


# ---- 1. logits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("B,D,C", [(1, 64, 2), (5, 70, 6), (65, 512, 101), (130, 768, 128), (3, 101, 65)])
def test_logits_equal_head_logits_bit_for_bit(ops, M, B, D, C):
    """Dense normal features, weights and bias: logits_out[m] is ops.head_logits(x_m, W, b), bit for bit, in both modes."""
    seed = 9100 + B + D + C
    feats = [O.portable_normal(seed + m, (B, D), stream=70).numpy() for m in range(M)]
    W = O.portable_normal(seed, (C, D), stream=71, std=0.05).numpy()
    b = O.portable_normal(seed, (C,), stream=72, std=0.1).numpy()
    label = O.portable_labels(seed, B, C).numpy()
    ref = []
    for f in feats:
        out = torch.full((B, C), float("nan"), device="cuda")
        ops.head_logits(dev(f), dev(W), dev(b), out)
        ref.append(out.cpu().numpy())
    for mode in (0, 1):
        got = run_head(ops, feats, W, b, label, mode, T.EVAL_ALPHAS[M])
        for m in range(M):
            same_bits(got.logits[m], ref[m], f"mode {mode} logits_out[{m}] vs head_logits")
        assert got.counts[0].sum() == B


# ---- 2. fixed mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("B", [1, 3, 5, 65, 257])
@pytest.mark.parametrize("C", [2, 6, 101])
def test_fixed_mode_counts_are_exact_and_equal_eval_fuse(ops, M, B, C):
    """Integer logits with forced ties, alphas (0.5, 0.5) / (0.5, 0.25, 0.25): the fused values are exact and the arg-max is the first
    maximum.  The counters equal the model's and ops.eval_fuse's on the same logits; a second call doubles them."""
    outs, label = T.eval_fixed_case(M, B, C)
    al = T.EVAL_ALPHAS[M]
    want = T.eval_counts(outs, label, al)
    m = E.eval_rows(outs, label, 0, al)
    assert (m.counts == want).all()
    got = through_identity(ops, outs, label, 0, al)
    assert (got.counts == want).all(), (got.counts, want)
    assert (got.pred == m.pred).all()
    assert got.pred[0].tolist() == [0] * (1 + M) and got.pred[B // 2, 1] == int(np.argmax(outs[0][B // 2]))     # the forced ties
    same_bits(got.weights, np.tile(np.array(al, dtype=F32), (B, 1)), "fixed weights")
    same_bits(got.fused, m.fused.astype(F32), "fixed fused (exact)")
    fuse_counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    ops.eval_fuse([got.logits_dev[k] for k in range(M)], dev(label, torch.int64), fuse_counts, torch.zeros(3, device="cuda"), False, list(al))
    assert (fuse_counts.view(2 + M, C).cpu().numpy() == got.counts).all()
    twice = through_identity(ops, outs, label, 0, al, calls=2)
    assert (twice.counts == 2 * want).all()


# ---- 3. sample mode, dense -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,C", E.SAMPLE_DENSE)
def test_sample_mode_dense(ops, M, B, C):
    """Weights within 1e-5 of fp64, fused logits within M * 1e-5 * max |logit|, counters and arg-maxes exact, row sums within 1e-6.
    Measured on an MI355X over the eight cases: weights off by at most 2.1e-7, fused by 1.04e-6 (bounds 4.4e-5 to 2.0e-4), row sums by
    8.9e-8; the worst of each at (3, 130, 128) resp. (2, 32, 6)."""
    outs, label = E.sample_dense_case(M, B, C)
    m = E.eval_rows(outs, label, 1, T.EVAL_ALPHAS[M])
    assert E.top2_margin(m.fused) >= E.EVAL_MARGIN              # every row; tests/test_eval_head_cpu.py prints the margins
    got = through_identity(ops, outs, label, 1, T.EVAL_ALPHAS[M])
    check_against_model(got, m, M, outs, f"sample dense M={M} B={B} C={C}")


# ---- 4. designed rows ------------------------------------------------------------------------------------------------------------------
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@pytest.mark.parametrize("C", [6, 65, 101])
def test_designed_rows(ops, C):
    """One batch, M = 3.  Row 0: the same logits in every modality.  Rows 1-3: one saturated modality (a logit 200 above the rest, at
    the last class) against two uniform ones, at each position.  Rows 4-9: three dense rows in all six orders."""
    x = [O.portable_normal(9300 + C + k, (C,), stream=73, std=1.5).numpy() for k in range(3)]
    uni, sat = np.zeros(C, dtype=F32), E.saturated_row(C, C - 1)
    rows = [[x[0], x[0], x[0]]]
    rows += [[sat if m == k else uni for m in range(3)] for k in range(3)]
    rows += [[x[p[m]] for m in range(3)] for p in PERMS]
    outs = [np.stack([r[m] for r in rows]).astype(F32) for m in range(3)]
    label = np.full(len(rows), C - 1, dtype=np.int64)
    got = through_identity(ops, outs, label, 1, ALPHAS3)
    w = got.weights
    assert bits(w[0])[0] == bits(w[0])[1] == bits(w[0])[2] and abs(float(w[0, 0]) - 1 / 3) <= 1e-6
    for k in range(3):
        r = 1 + k
        print(f"saturated at modality {k}, C={C}: weights {w[r]}, want {C / (C + 2):.7f}")
        assert abs(float(w[r, k]) - C / (C + 2)) <= E.WEIGHT_TOL
        assert got.pred[r].tolist() == [C - 1] + [C - 1 if m == k else 0 for m in range(3)]      # the uniform ones answer class 0
        same_bits(np.roll(w[r], -k), w[1], "the saturated rows are rotations of row 1")
    for i, p in enumerate(PERMS):                                 # modality m of row 4 + i holds x[p[m]]
        same_bits(w[4 + i], w[4][list(p)], f"permutation {p}")
    m = E.eval_rows(outs, label, 1, ALPHAS3)
    assert E.top2_margin(m.fused) >= E.EVAL_MARGIN
    check_against_model(got, m, 3, outs, f"designed rows C={C}")


# ---- 5. batch independence -------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_batch_split(ops):
    M, B, C = 3, 65, 101
    outs, label = E.sample_dense_case(M, B, C)
    whole = through_identity(ops, outs, label, 1, ALPHAS3)
    for sizes in ([64, 1], [13] * 5):
        counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
        parts, o = [], 0
        for n in sizes:
            parts.append(through_identity(ops, [x[o:o + n] for x in outs], label[o:o + n], 1, ALPHAS3, counts=counts))
            o += n
        assert o == B
        assert (parts[-1].counts == whole.counts).all()
        same_bits(np.concatenate([p.weights for p in parts]), whole.weights, f"weights_out in batches of {sizes}")
        same_bits(np.concatenate([p.fused for p in parts]), whole.fused, f"fused_out in batches of {sizes}")
        assert (np.concatenate([p.pred for p in parts]) == whole.pred).all()


# ---- 6. presence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_presence(ops, mode):
    """M = 3, B = 65, every non-empty pattern; row 7 has no modality, rows 0 and B - 1 carry the labels -1 and C."""
    M, B, C = 3, 65, 101
    outs, label = E.sample_dense_case(M, B, C)
    label = label.copy()
    label[0], label[B - 1] = -1, C
    present = E.every_pattern(B)
    present[7] = 0
    m = E.eval_rows(outs, label, mode, ALPHAS3, present=present)
    assert m.bad.tolist() == [r in (0, 7, B - 1) for r in range(B)] and m.counts[0].sum() == B - 3
    assert E.top2_margin(m.fused) >= E.EVAL_MARGIN
    assert {tuple(p) for p in present.tolist()} == {tuple((q >> k) & 1 for k in range(3)) for q in range(8)}
    got = through_identity(ops, outs, label, mode, ALPHAS3, present=present)
    check_against_model(got, m, M, outs, f"presence mode {mode}")
    ok = ~m.bad
    absent = (present == 0) & ok[:, None]
    assert (bits(got.weights)[absent] == 0).all()                              # exactly +0.0
    if mode == 0:
        al = np.array(ALPHAS3, dtype=F64)
        want = np.where(present != 0, al, 0) / np.where(present != 0, al, 0).sum(axis=1, keepdims=True).clip(1e-30)
        assert np.abs(got.weights[ok].astype(F64) - want[ok]).max() <= E.WEIGHT_TOL
        full = ok & (present != 0).all(axis=1)
        same_bits(got.weights[full], np.tile(np.array(ALPHAS3, dtype=F32), (int(full.sum()), 1)), "rows with every modality keep the alphas")
    # the absent modality's own prediction and counter are those of its logits
    for k in range(M):
        assert (got.pred[ok, 1 + k] == outs[k][ok].argmax(axis=1)).all()
        hit = ok & (outs[k].argmax(axis=1) == label)
        assert (got.counts[2 + k] == np.bincount(label[hit], minlength=C)).all()
    # every other row is what it is without the bad rows around it
    alone = through_identity(ops, [o[1:7] for o in outs], label[1:7], mode, ALPHAS3, present=present[1:7])
    same_bits(alone.weights, got.weights[1:7], "rows 1-6 alone")
    same_bits(alone.fused, got.fused[1:7], "rows 1-6 alone")


def test_fixed_mode_row_whose_present_modalities_carry_no_share_is_a_bad_row(ops):
    """alphas (1, 0, 0): a row without modality 0 has eligible alphas summing to 0, nothing to renormalise by.  It is counted nowhere
    (NaN weights, pred -1) instead of dividing by zero; the rows around it are intact, a full row keeps its alphas."""
    M, C = 3, 6
    outs, label = E.sample_dense_case(M, 4, C)
    present = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 0], [1, 1, 0]], dtype=np.uint8)
    m = E.eval_rows(outs, label, 0, (1.0, 0.0, 0.0), present=present)
    assert m.bad.tolist() == [False, True, False, False] and E.top2_margin(m.fused) >= E.EVAL_MARGIN
    got = through_identity(ops, outs, label, 0, (1.0, 0.0, 0.0), present=present)
    check_against_model(got, m, M, outs, "no share left")
    same_bits(got.weights[[0, 2, 3]], np.tile(np.array([1, 0, 0], dtype=F32), (3, 1)), "weights of the good rows")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,match", [("C129", "need 0 < C <= 128"), ("M1", "need M = 2 or 3"), ("mode2", "need mode = 0"),
                                        ("null", "null pointer")])
def test_refusals_launch_nothing(ops, what, match):
    from mla_hip._lib import MLAHipError
    M, B, D = (1 if what == "M1" else 2), 5, 64
    C = 129 if what == "C129" else 6
    ar = Arena()
    logits, fused, weights, pred = ar.f32(M, B, C), ar.f32(B, C), ar.f32(B, M), ar.i32(B, 1 + M)
    counts = ar.i32(C * (2 + M))
    feats = [torch.zeros((B, D), device="cuda") for _ in range(M)]
    with pytest.raises(MLAHipError, match=match):
        ops.eval_head(feats, torch.zeros((C, D), device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(B, device="cuda", dtype=torch.int64),
                      counts, None if what == "null" else logits, mode=2 if what == "mode2" else 1, alphas=[0.5, 0.5], fused_out=fused,
                      weights_out=weights, pred_out=pred)
    ar.check(written=False)


# ---- 8. Evaluator ----------------------------------------------------------------------------------------------------------------------
class _ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


def _clip_data(n_batches=2, B=10, D=64):
    tok = O.portable_normal(9400, (n_batches * B, 1, D), stream=74)
    img = O.portable_normal(9401, (n_batches * B, 1, D), stream=75)
    return tok, img, O.portable_labels(9400, n_batches * B, 6)


def _clip_model():
    from mla_hip import CLIPClassifier
    model = CLIPClassifier(_ClipArgs(), seed=3, feat_dim=64)
    with torch.no_grad():                                   # a head that separates the classes: logits of order 1
        model.fusion_module.fc_out.weight.copy_(O.portable_normal(9402, (6, 64), stream=76, std=0.2))
        model.fusion_module.fc_out.bias.copy_(O.portable_normal(9403, (6,), stream=77, std=0.1))
    return model


def _logits64(model, feats):
    W, b = model.fusion_module.fc_out.weight.detach().cpu().double().numpy(), model.fusion_module.fc_out.bias.detach().cpu().double().numpy()
    return [f.double().numpy().reshape(f.shape[0], -1) @ W.T + b for f in feats]


def test_evaluator_sample_mode_equals_the_restatement_and_one_batch():
    from mla_hip import Evaluator
    model, (tok, img, label), B = _clip_model(), _clip_data(), 10
    outs = _logits64(model, (tok, img))
    m = E.eval_rows(outs, label.numpy(), 1, (0.5, 0.5))
    for f in [m.fused] + outs:                              # the fused and each modality's arg-max stand clear of fp32 rounding
        assert E.top2_margin(f) >= E.EVAL_MARGIN
    ev = Evaluator(model, dynamic=True, dynamic_mode="sample")
    for s in (slice(0, B), slice(B, 2 * B)):
        got = ev.update(tok[s].cuda(), img[s].cuda(), label[s].cuda())
        assert len(got) == 2 and got[0].shape == (B, 6) and got[0].data_ptr() == ev._sample_bufs(B)["logits"].data_ptr()
        assert np.abs(ev.sample_weights.cpu().numpy().astype(F64) - m.weights[s]).max() <= E.WEIGHT_TOL
        assert (ev.pred.cpu().numpy() == m.pred[s]).all()
        assert np.abs(ev.fused.cpu().numpy().astype(F64) - m.fused[s]).max() <= E.fused_tol(2, outs)
        assert np.abs(got[1].cpu().numpy().astype(F64) - outs[1][s]).max() <= 2e-6 * (1 + np.abs(outs[1]).max())
    assert (ev.per_class() == m.counts).all() and ev.per_class().dtype == np.int64
    tot = m.counts.sum(axis=1)
    assert ev.result() == tuple(tot[1:] / tot[0])
    one = Evaluator(model, dynamic=True, dynamic_mode="sample")
    one.update(tok.cuda(), img.cuda(), label.cuda())
    assert (one.per_class() == ev.per_class()).all() and one.result() == ev.result()
    ev.reset()
    assert ev.per_class().sum() == 0


def test_evaluator_default_path_is_the_published_chain():
    from mla_hip import Evaluator, ops
    model, (tok, img, label) = _clip_model(), _clip_data()
    head = model.fusion_module.fc_out
    for dynamic in (True, False):
        ev = Evaluator(model, dynamic=dynamic)
        ev.update(tok.cuda(), img.cuda(), label.cuda())
        assert not ev.per_sample and not hasattr(ev, "sample_weights")
        outs = []
        for f in (tok, img):
            out = torch.empty((f.shape[0], 6), device="cuda")
            ops.head_logits(f.squeeze(1).cuda().contiguous(), head.weight.detach(), head.bias.detach(), out)
            outs.append(out)
        counts, w = torch.zeros(6 * 4, device="cuda", dtype=torch.int32), torch.zeros(3, device="cuda")
        ops.eval_fuse(outs, label.cuda(), counts, w, dynamic, [0.5, 0.5])
        assert torch.equal(ev.counts, counts) and torch.equal(ev.weights, w)
        assert (ev.per_class() == counts.view(4, 6).cpu().numpy()).all()


@pytest.mark.parametrize("dynamic", [False, True])
def test_evaluator_gate_absent_on_modal3classifier(ops, dynamic):
    """The real three-modality model (depth 2, the inputs of tests/test_modal3_present_gpu.py): what Evaluator leaves behind is, bit
    for bit, what a direct call produces from the logits it returned (through the identity head) with the mask's columns on
    (a, v, t); another pairing of the columns gives other weights.  Without gate_absent, present= only skips rows in the encoders."""
    import test_modal3_present_gpu as P
    from mla_hip import Evaluator
    mask = np.array(P.MASKS["mixed"], dtype=np.uint8)
    inputs, label = P._inputs(mask.tolist())
    ev = Evaluator(P._model(), dynamic=dynamic, dynamic_mode="sample", gate_absent=True)
    outs = [o.cpu().numpy() for o in ev.update(*inputs, label, present=torch.from_numpy(mask))]
    mode = 1 if dynamic else 0
    want = through_identity(ops, outs, label.cpu().numpy(), mode, ALPHAS3, present=mask)
    w = ev.sample_weights.cpu().numpy()
    same_bits(w, want.weights, "Evaluator.sample_weights")
    same_bits(ev.fused.cpu().numpy(), want.fused, "Evaluator.fused")
    assert (ev.pred.cpu().numpy() == want.pred).all() and (ev.per_class() == want.counts).all()
    assert (bits(w)[mask == 0] == 0).all() and (w[mask != 0] > 0).all() and np.abs(w.sum(axis=1) - 1).max() <= 1e-6
    other = through_identity(ops, outs, label.cpu().numpy(), mode, ALPHAS3, present=mask[:, [1, 0, 2]])
    assert (bits(other.weights) != bits(w)).any()
    plain = Evaluator(P._model(), dynamic=True, dynamic_mode="sample")
    plain.update(*inputs, label, present=torch.from_numpy(mask))
    assert (plain.sample_weights.cpu().numpy() > 0).all() and int(plain.per_class()[0].sum()) == P.B


class StubModal3:
    """What Evaluator asks of a three-modality model whose forward takes present=: the features are handed in directly, in
    mla_encoders() order (a, v, t), and the head is the identity, so the logits are the features."""

    def __init__(self, C):
        from mla_hip.model import SharedHead
        self.device = torch.device("cuda")
        self.fusion_module = SimpleNamespace(fc_out=SharedHead(C, C, "cuda", seed=0))
        W, b = E.identity_head(C)
        with torch.no_grad():
            self.fusion_module.fc_out.weight.copy_(torch.from_numpy(W))
            self.fusion_module.fc_out.bias.copy_(torch.from_numpy(b))

    def mla_encoders(self):
        return [("a", "audio", None), ("v", "image", None), ("t", "text", None)]

    def forward_raw(self, *inputs, present=None):
        return tuple(inputs)

    def eval(self):
        return self


@pytest.mark.parametrize("dynamic", [False, True])
def test_evaluator_gate_absent_puts_the_columns_on_the_right_modalities(dynamic):
    from mla_hip import Evaluator
    M, B, C = 3, 64, 4
    outs, label = E.sample_dense_case(M, B, C)
    present = E.every_pattern(B)
    swapped = present[:, [1, 0, 2]]
    mode = 1 if dynamic else 0
    m = E.eval_rows(outs, label, mode, ALPHAS3, present=present)
    other = E.eval_rows(outs, label, mode, ALPHAS3, present=swapped)
    assert (m.counts != other.counts).any()                 # swapping two columns changes the counters
    assert E.top2_margin(m.fused) >= E.EVAL_MARGIN
    ev = Evaluator(StubModal3(C), dynamic=dynamic, dynamic_mode="sample", gate_absent=True)
    ev.update(*[dev(o) for o in outs], dev(label, torch.int64), present=torch.from_numpy(present))
    assert (ev.per_class() == m.counts).all()
    assert np.abs(ev.sample_weights.cpu().numpy().astype(F64) - m.weights).max() <= E.WEIGHT_TOL
    assert (bits(ev.sample_weights.cpu().numpy())[present == 0] == 0).all()
    # without present= every modality takes part
    full = Evaluator(StubModal3(C), dynamic=dynamic, dynamic_mode="sample", gate_absent=True)
    full.update(*[dev(o) for o in outs], dev(label, torch.int64))
    assert (full.per_class() == E.eval_rows(outs, label, mode, ALPHAS3).counts).all()
