"""csrc/metrics.hip on the GPU: the score store's append launch, average precision without a sort, confusion counts, and the three
evaluators with metrics=True, against the fp64 restatement of tests/metrics_model.py.

  exact (bit for bit)   ap against ap_ordered (the kernel's order is the definition), its per-row terms, npos; confusion counts; pred
                        (first maximum of the logits); labels; saturated and equal-logit score rows; head 0 formed from the weight
                        vector against the same fused logits passed as a matrix, on exactly-summable inputs; the diagonal of
                        confusion() against the evaluators' own counters; everything a metrics=False twin produces
  derived bound         stored probabilities against the fp64 softmax under exact_tokens.softmax_tol, the bound
                        tests/test_head_exact_gpu.py holds the dense softmax rows of tests/head_exact.py to

Every output starts filled (a NaN no kernel produces; -7 for integers) inside guarded buffers: each call writes what it should and
nothing else.  Rows past N of every store are poison (NaN scores under valid labels): a kernel that read one would change npos."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_exact as HX  # noqa: E402
import metrics_model as MM  # noqa: E402
from exact_tokens import softmax_tol  # noqa: E402
from oracle import mla_oracle as O  # noqa: E402

F32, F64 = np.float32, np.float64
FILL = 0x7FC0BEEF          # a quiet NaN no kernel produces
IFILL = -7
GUARD = 256


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(device="cuda", dtype=dtype).contiguous()


class Arena:
    """Guarded, filled device buffers of one call: 4-byte words (fp32: the NaN pattern, int32: -7) and fp64 (both words the pattern)."""

    def __init__(self):
        self.bufs = []

    def _new(self, shape, fill, words):
        n = math.prod(shape) * words
        flat = torch.full((n + 2 * GUARD,), fill, dtype=torch.int32, device="cuda")
        self.bufs.append((flat, n, fill))
        return flat[GUARD:GUARD + n]

    def f32(self, *shape):
        return self._new(shape, FILL, 1).view(torch.float32).view(shape)

    def i32(self, *shape):
        return self._new(shape, IFILL, 1).view(shape)

    def f64(self, *shape):
        return self._new(shape, FILL, 2).view(torch.float64).view(shape)

    def guards_intact(self):
        torch.cuda.synchronize()
        for flat, n, fill in self.bufs:
            assert bool((flat[:GUARD] == fill).all()) and bool((flat[GUARD + n:] == fill).all()), "a guard was overwritten"


def unwritten64(t):
    """Which fp64 elements still hold the fill in both words."""
    return (t.contiguous().view(torch.int32).view(*t.shape, 2) == FILL).all(dim=-1).cpu().numpy()


def same_f64(got, want, name):
    """Bit for bit; NaN where and only where the model has NaN (a NaN's payload is not part of the contract)."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape, f"{name}: {got.shape} vs {want.shape}"
    assert (np.isnan(got) == np.isnan(want)).all(), f"{name}: NaN at {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
    ok = ~np.isnan(want)
    bad = np.flatnonzero(got[ok].view(np.int64) != want[ok].view(np.int64))
    assert bad.size == 0, f"{name}: {bad.size} of {ok.sum()} differ, first {got[ok][bad[0]]!r} vs {want[ok][bad[0]]!r}"


def same_f32(got, want, name):
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert got.shape == want.shape, f"{name}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got.view(np.int32).ravel() != want.view(np.int32).ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


# ---- 1. average precision on given score matrices ---------------------------------------------------------------------------------------
def run_ap(ops, scores, labels, N):
    H, C, cap = scores.shape
    ar = Arena()
    ap, npos, ws = ar.f64(H, C), ar.i32(C), ar.f64(H, cap)
    ops.average_precision(dev(scores), dev(labels, torch.int32), N, ap, npos, ws)
    ar.guards_intact()
    return ap.cpu().numpy(), npos.cpu().numpy(), ws.cpu().numpy(), unwritten64(ws)


@pytest.mark.parametrize("H", MM.AP_H)
@pytest.mark.parametrize("C", MM.AP_C)
@pytest.mark.parametrize("N", MM.AP_N)
def test_average_precision_equals_the_ordered_restatement_bit_for_bit(ops, N, C, H):
    for family in MM.AP_FAMILIES:
        scores, labels = MM.ap_case(N, C, H, family)
        assert scores.shape[2] > N and np.isnan(scores[:, :, N:]).all() and (labels[N:] >= 0).all() and (labels[N:] < C).all()
        want_ap, want_npos, want_terms = MM.ap_ordered(scores, labels, N)
        ap, npos, ws, untouched = run_ap(ops, scores, labels, N)
        name = f"{family} N={N} C={C} H={H}"
        assert (npos == want_npos).all(), f"{name}: npos {npos.tolist()} vs {want_npos.tolist()}"
        same_f64(ws[:, :N], want_terms, f"{name} terms")
        assert untouched[:, N:].all() and not untouched[:, :N].any(), f"{name}: the terms of rows >= N were written"
        same_f64(ap, want_ap, f"{name} ap")
        if C >= 3 and N >= 2:
            assert want_npos[1] == 0 and np.isnan(ap[:, 1]).all()            # a class without a positive
        if C == 1 and family != "special":
            assert want_npos[0] == N                                          # a class that is all positives
            if family == "quarters":                                          # every positive's term is 1: AP = 1
                assert (ap == 1.0).all()


def test_average_precision_policies(ops):
    """NaN-scored positives contribute 0, labels -1 and C are positives of no class and negatives of every class, +-inf order like
    numbers: the hand-computed case of tests/test_metrics_cpu.py, on the device."""
    scores = np.array([[[0.5, np.nan, 0.25, 0.5, 0.75, np.nan], [0.1, 0.2, np.nan, 0.4, 0.5, np.nan]]], dtype=F32)
    labels = np.array([0, 0, 1, 7, -1, 0], dtype=np.int32)
    ap, npos, ws, _ = run_ap(ops, scores, labels, 5)
    assert ws[0, :5].tolist() == [1 / 3, 0.0, 0.0, 0.0, 0.0] and npos.tolist() == [2, 1]
    assert ap[0, 0] == (1 / 3 + 0.0) / 2 and ap[0, 1] == 0.0
    s = np.array([[[np.inf, -np.inf, 0.0, np.inf]]], dtype=F32)
    ap, npos, ws, _ = run_ap(ops, s, np.zeros(4, dtype=np.int32), 4)
    assert ws[0].tolist() == [1.0, 1.0, 1.0, 1.0] and ap[0, 0] == 1.0 and npos.tolist() == [4]


def test_average_precision_and_confusion_torch_ops_on_own_scores(ops):
    N, C, H = 130, 6, 3
    scores, labels = MM.ap_case(N, C, H, "quarters")
    s, lab = np.ascontiguousarray(scores[:, :, :N]), labels[:N]
    want, _, _ = MM.ap_ordered(s, lab, N)
    got = torch.ops.mla_hip.average_precision(dev(s), dev(lab, torch.int64))
    assert got.dtype == torch.float64 and got.shape == (H, C)
    same_f64(got.cpu().numpy(), want, "torch op ap")
    one = torch.ops.mla_hip.average_precision(dev(s[1]), dev(lab, torch.int32))
    same_f64(one.cpu().numpy(), want[1], "torch op ap, one head")
    pred = np.random.default_rng(5).integers(-1, C + 1, size=(H, N)).astype(np.int32)
    conf = torch.ops.mla_hip.confusion_count(dev(pred), dev(lab, torch.int64), C)
    assert conf.dtype == torch.int32 and (conf.cpu().numpy() == MM.confusion(pred, lab, N, C)).all()
    assert (torch.ops.mla_hip.confusion_count(dev(pred[2]), dev(lab, torch.int64), C).cpu().numpy() == MM.confusion(pred, lab, N, C)[2]).all()


# ---- 2. confusion counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", MM.AP_H)
@pytest.mark.parametrize("N,C", [(1, 1), (63, 2), (65, 6), (130, 65), (300, 128), (1000, 3)])
def test_confusion_counts_are_exact(ops, N, C, H):
    rng = np.random.default_rng(100 * N + C + H)
    cap = N + MM.TAIL
    pred = rng.integers(0, C, size=(H, cap)).astype(np.int32)
    labels = rng.integers(0, C, size=cap).astype(np.int32)
    if N >= 63:
        labels[[0, N - 1]] = -1, C                                            # skipped for every head
        pred[0, 5], pred[H - 1, 6] = -1, C                                    # skipped for that head
    ar = Arena()
    conf = ar.i32(H, C, C)
    conf.zero_()
    want = MM.confusion(pred, labels, N, C)
    for calls in (1, 2):                                                      # accumulated: a second call doubles
        ops.confusion_count(dev(pred), dev(labels), N, conf)
        ar.guards_intact()
        assert (conf.cpu().numpy() == calls * want).all()
    bad = 2 * H + 2 if N >= 63 else 0
    assert want.sum() == H * N - bad


# ---- 3. append --------------------------------------------------------------------------------------------------------------------------
def append_case(H, C):
    """H logit matrices (73, C), one head_exact dense cross-entropy family per head, and labels; batches MM.APPEND_BATCHES."""
    B = sum(MM.APPEND_BATCHES)
    logits = [HX.dense_ce_case(B, C, HX.CE_FAMILIES[(h + C) % len(HX.CE_FAMILIES)]).logits.numpy() for h in range(H)]
    labels = O.portable_labels(700 + C, B, C).numpy().astype(np.int64)
    return logits, labels


def new_store(H, C, cap):
    ar = Arena()
    return ar, ar.f32(H, C, cap), ar.i32(H, cap), ar.i32(cap)


@pytest.mark.parametrize("H", [1, 3, 4])
@pytest.mark.parametrize("C", [1, 2, 6, 65, 128])
def test_append_fills_exactly_its_rows(ops, H, C):
    logits, labels = append_case(H, C)
    cap = MM.APPEND_CAP
    ar, scores, pred, lab = new_store(H, C, cap)
    d_logits, d_labels = [dev(l) for l in logits], dev(labels)
    pos = 0
    for B in MM.APPEND_BATCHES:                                               # offsets 0, 1, 6, 70; the last batch is short
        ops.scores_append([l[pos:pos + B] for l in d_logits], d_labels[pos:pos + B], scores, pred, lab, pos)
        pos += B
        ar.guards_intact()
        assert bool((lab[pos:] == IFILL).all()) and bool((pred[:, pos:] == IFILL).all())          # nothing past the batch
        assert bool((scores[:, :, pos:].contiguous().view(torch.int32) == FILL).all())
    got, n = scores.cpu().numpy(), pos
    assert n == 73 and n < cap
    for h in range(H):
        ref = MM.softmax64(logits[h])                                         # (n, C)
        err, tol = float(np.abs(got[h, :, :n].T.astype(F64) - ref).max()), softmax_tol(torch.from_numpy(ref))
        print(f"H={H} C={C} head {h}: stored probabilities off the fp64 softmax by {err:.3g} (bound {tol:.3g})")
        assert err <= tol
        assert (pred[h, :n].cpu().numpy() == MM.first_argmax(logits[h])).all()
    assert (lab[:n].cpu().numpy() == labels).all()


@pytest.mark.parametrize("C", [1, 2, 64, 65, 128])
def test_append_saturated_equal_and_tied_rows_are_exact(ops, C):
    """Saturated row: the winner's probability is exactly 1, every other exactly 0 (exp(-128) is 0 in fp32).  Equal row: fl(1 / C) in
    every class.  pred is the first maximum of the LOGITS, ties included; labels -1 and C are copied as they are."""
    rows, want, arg = [], [], []
    for win in sorted({0, C // 2, C - 1}):
        r = np.full(C, -3.0, dtype=F32)
        r[win] = 125.0
        rows.append(r), want.append(np.eye(C, dtype=F32)[win]), arg.append(win)
    for v in (0.75, -1e4):
        rows.append(np.full(C, v, dtype=F32)), want.append(np.full(C, F32(1) / F32(C), dtype=F32)), arg.append(0)
    if C >= 3:                                                                # two equal maxima: the first wins
        r = np.zeros(C, dtype=F32)
        r[[C - 1, 1]] = 2.0
        rows.append(r), want.append(None), arg.append(1)
    logits, B = np.stack(rows), len(rows)
    labels = np.arange(B, dtype=np.int64) % C
    labels[0], labels[-1] = -1, C
    ar, scores, pred, lab = new_store(2, C, B + 3)
    ops.scores_append([dev(logits), dev(logits[::-1].copy())], dev(labels), scores, pred, lab, 2)
    ar.guards_intact()
    got = scores.cpu().numpy()
    for r in range(B):
        if want[r] is not None:
            same_f32(got[0, :, 2 + r], want[r], f"C={C} row {r}")
            same_f32(got[1, :, 2 + B - 1 - r], want[r], f"C={C} row {r}, second head")
    assert pred[0, 2:2 + B].cpu().tolist() == arg and pred[1, 2:2 + B].cpu().tolist() == arg[::-1]
    assert lab[2:2 + B].cpu().tolist() == labels.tolist() and lab[:2].cpu().tolist() == [IFILL, IFILL] and int(lab[-1]) == IFILL


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("C", [2, 6, 65, 128])
def test_append_forms_head_0_from_the_weight_vector(ops, M, C):
    """Quarter-valued logits and power-of-two weights: sum_m w_m l_m is exact in fp32 in any order, so head 0 formed in the kernel
    equals, bit for bit, the same fused logits passed as a matrix, and the modality heads do not depend on the form."""
    B = 70
    w = np.array([0.5, 0.25, 0.25][:M] if M == 3 else [0.5, 0.5], dtype=F32)
    rng = np.random.default_rng(40 + M + C)
    outs = [(rng.integers(-12, 13, size=(B, C)) / 4).astype(F32) for _ in range(M)]
    fused = sum(w[m] * outs[m] for m in range(M)).astype(F32)
    assert (fused.astype(F64) == sum(w[m].astype(F64) * outs[m].astype(F64) for m in range(M))).all()
    labels = rng.integers(0, C, size=B).astype(np.int64)
    stores = []
    for form in ("weights", "matrix"):
        ar, scores, pred, lab = new_store(1 + M, C, B + 2)
        first = None if form == "weights" else dev(fused)
        ops.scores_append([first] + [dev(o) for o in outs], dev(labels), scores, pred, lab, 1,
                          weights=dev(np.concatenate([w, [9.0]]).astype(F32)[:3]) if form == "weights" else None)
        ar.guards_intact()
        stores.append((scores.cpu().numpy(), pred.cpu().numpy(), lab.cpu().numpy()))
    same_f32(stores[0][0], stores[1][0], f"M={M} C={C} scores, weights form vs matrix form")
    assert (stores[0][1] == stores[1][1]).all() and (stores[0][2] == stores[1][2]).all()
    assert (stores[0][1][0, 1:1 + B] == MM.first_argmax(fused)).all()
    ref = MM.softmax64(fused)
    assert np.abs(stores[0][0][0, :, 1:1 + B].T.astype(F64) - ref).max() <= softmax_tol(torch.from_numpy(ref))


@pytest.mark.parametrize("M,alphas", [(2, (0.35, 0.65)), (3, (0.35, 0.25, 0.4))])
def test_append_head_0_follows_eval_fuse_through_near_ties(ops, M, alphas):
    """The store's head 0 is formed with eval_fuse_kernel's expression and order: on rows whose two leading fused values lie within
    two ulps of each other -- where another rounding of the sum flips the arg-max, as the two roundings of fuse32 show -- the diagonal
    of the confusion counts equals eval_fuse's fused-correct counters per class, and so do the modality heads'."""
    B, C = 512, 6
    outs, labels, w = MM.near_tie_case(M, B, C, alphas)
    flips = int((MM.first_argmax(MM.fuse32(outs, w, True)) != MM.first_argmax(MM.fuse32(outs, w, False))).sum())
    print(f"M={M}: the two roundings of the fused sum disagree on {flips} of {B} rows")
    assert flips >= 16
    d_outs, d_labels = [dev(o) for o in outs], dev(labels)
    counts, used = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32), torch.zeros(3, device="cuda")
    ops.eval_fuse(d_outs, d_labels, counts, used, False, list(alphas))
    assert used[:M].cpu().tolist() == w.tolist()
    ar, scores, pred, lab = new_store(1 + M, C, B)
    ops.scores_append([None] + d_outs, d_labels, scores, pred, lab, 0, weights=used)
    conf = torch.zeros((1 + M, C, C), device="cuda", dtype=torch.int32)
    ops.confusion_count(pred, lab, B, conf)
    ar.guards_intact()
    c, conf = counts.view(2 + M, C).cpu().numpy(), conf.cpu().numpy()
    for h in range(1 + M):
        assert (np.diag(conf[h]) == c[1 + h]).all(), (h, np.diag(conf[h]), c[1 + h])
        assert (conf[h].sum(axis=1) == c[0]).all()


def test_append_overflow_raises_and_leaves_the_store_byte_identical(ops):
    from mla_hip import ScoreStore
    from mla_hip._lib import MLAHipError
    H, C, cap = 3, 6, 10
    logits, labels = append_case(H, C)
    ar, scores, pred, lab = new_store(H, C, cap)
    d = [dev(l) for l in logits]
    ops.scores_append([l[:6] for l in d], dev(labels[:6]), scores, pred, lab, 0)
    torch.cuda.synchronize()
    before = [t.clone() for t in (scores.view(torch.int32), pred, lab)]
    for pos, B in ((6, 5), (10, 1), (0, 11), (-1, 2)):
        with pytest.raises(MLAHipError, match="do not fit"):
            ops.scores_append([l[:B] for l in d], dev(labels[:B]), scores, pred, lab, pos)
    ar.guards_intact()
    assert all(torch.equal(a, b) for a, b in zip(before, (scores.view(torch.int32), pred, lab)))
    ops.scores_append([l[6:10] for l in d], dev(labels[6:10]), scores, pred, lab, 6)        # exactly full is fine
    ar.guards_intact()
    assert not bool((lab == IFILL).any())
    st = ScoreStore(H, C, cap, "cuda")                                        # the store refuses on the host, before the entry point
    st.append([l[:8] for l in d], dev(labels[:8]))
    keep = [t.clone() for t in (st.scores, st.pred, st.labels)]
    with pytest.raises(MLAHipError, match="capacity=10"):
        st.append([l[:3] for l in d], dev(labels[:3]))
    torch.cuda.synchronize()
    assert st.n == 8 and all(torch.equal(a, b) for a, b in zip(keep, (st.scores, st.pred, st.labels)))


# ---- 4. the evaluators ------------------------------------------------------------------------------------------------------------------
class _ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


class _JointClipArgs(_ClipArgs):
    gs_flag = False


class _AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
    lorb, clip, modal3 = "base", False, False


N_BATCHES, BATCH, DIM, CLASSES = 2, 10, 64, 6


def _clip_data():
    tok = O.portable_normal(9400, (N_BATCHES * BATCH, 1, DIM), stream=74)
    img = O.portable_normal(9401, (N_BATCHES * BATCH, 1, DIM), stream=75)
    return tok.cuda(), img.cuda(), O.portable_labels(9400, N_BATCHES * BATCH, CLASSES).cuda()


def _clip_model(args):
    from mla_hip import CLIPClassifier
    model = CLIPClassifier(args(), seed=3, feat_dim=DIM)
    with torch.no_grad():                                   # a head that separates the classes: logits of order 1
        head = model.fusion_module.fc_out
        head.weight.copy_(O.portable_normal(9402, tuple(head.weight.shape), stream=76, std=0.2))
        head.bias.copy_(O.portable_normal(9403, tuple(head.bias.shape), stream=77, std=0.1))
    return model


def check_store_against_counters(ev, correct_rows, num_row, n):
    """correct_rows[h]: the evaluator's own correct-per-class counter of head h; num_row: its samples-per-class counter."""
    scores, pred, labels, got_n = ev.scores
    assert got_n == n and scores.shape[2] == n and ev._store.capacity > n
    conf = ev.confusion()
    H, C = conf.shape[0], conf.shape[1]
    assert conf.dtype == np.int64 and conf.shape == (H, C, C) and len(correct_rows) == H
    for h in range(H):
        assert (np.diag(conf[h]) == correct_rows[h]).all(), (h, np.diag(conf[h]), correct_rows[h])
        assert (conf[h].sum(axis=1) == num_row).all() and conf[h].sum() == n
    s, p, lab = scores.cpu().numpy(), pred.cpu().numpy(), labels.cpu().numpy()
    assert (conf == MM.confusion(p, lab, n, C)).all()
    for h in range(H):                                                        # every stored pred is a maximiser of its score row
        assert (s[h, p[h], np.arange(n)] == s[h].max(axis=0)).all()
    assert np.abs(s.sum(axis=1) - 1).max() <= 1e-6
    # average precision of the store, in the kernel's order; its mean over the classes that have a positive; F1 from the counts
    want_ap, npos, _ = MM.ap_ordered(np.ascontiguousarray(s), lab, n)
    ap = ev.average_precision()
    same_f64(ap, want_ap, "evaluator ap")
    assert ev.mean_average_precision() == tuple(float(np.mean(row[npos > 0])) for row in want_ap)
    for average in ("macro", "weighted"):
        assert ev.f1(average) == pytest.approx(tuple(MM.f1_scores(conf[h], average) for h in range(H)), abs=1e-15)
    return conf


@pytest.mark.parametrize("dynamic,mode", [(False, "batch"), (True, "batch"), (True, "sample")])
def test_evaluator_store_agrees_with_its_counters_and_metrics_false_is_unchanged(dynamic, mode):
    from mla_hip import Evaluator
    model, (tok, img, label) = _clip_model(_ClipArgs), _clip_data()
    n = N_BATCHES * BATCH
    ev = Evaluator(model, dynamic=dynamic, dynamic_mode=mode, metrics=True, capacity=n + 5)
    twin = Evaluator(model, dynamic=dynamic, dynamic_mode=mode)
    assert twin._store is None and twin._fixed_weights is None and ev.per_sample == (mode == "sample")
    for b in range(N_BATCHES):
        s = slice(b * BATCH, (b + 1) * BATCH)
        outs = [o.clone() for o in ev.update(tok[s], img[s], label[s])]
        outs_twin = twin.update(tok[s], img[s], label[s])
        assert all(torch.equal(a, c) for a, c in zip(outs, outs_twin))       # the returned logits, bit for bit
        assert torch.equal(ev.counts, twin.counts) and torch.equal(ev.weights, twin.weights)
        if ev.per_sample:
            assert torch.equal(ev.fused, twin.fused) and torch.equal(ev.pred, twin.pred)
            assert torch.equal(ev.sample_weights, twin.sample_weights)
    assert ev.result() == twin.result()
    pc = ev.per_class()                                                       # (2 + M, C): num, fused-correct, each modality's
    conf = check_store_against_counters(ev, [pc[1], pc[2], pc[3]], pc[0], n)
    assert tuple(np.trace(c) / n for c in conf) == ev.result()
    if ev.per_sample:                                                         # the stored head 0 is the kernel's own fused arg-max
        assert (ev.scores[1][0, BATCH:].cpu() == ev.pred[:, 0].cpu()).all()
    ev.reset()                                                                # restarts at row 0
    assert ev.scores[3] == 0 and ev.confusion().sum() == 0 and ev.per_class().sum() == 0
    ev.update(tok[:BATCH], img[:BATCH], label[:BATCH])
    assert ev.scores[3] == BATCH and ev.confusion().sum() == 3 * BATCH
    assert (np.diag(ev.confusion()[0]) == ev.per_class()[1]).all()


def test_evaluator_capacity_is_enforced_before_the_launch():
    from mla_hip import Evaluator
    from mla_hip._lib import MLAHipError
    model, (tok, img, label) = _clip_model(_ClipArgs), _clip_data()
    ev = Evaluator(model, metrics=True, capacity=BATCH + 3)
    ev.update(tok[:BATCH], img[:BATCH], label[:BATCH])
    torch.cuda.synchronize()
    keep = [t.clone() for t in (ev._store.scores, ev._store.pred, ev._store.labels)]
    with pytest.raises(MLAHipError, match="capacity=13"):
        ev.update(tok[BATCH:], img[BATCH:], label[BATCH:])
    torch.cuda.synchronize()
    assert ev.scores[3] == BATCH and all(torch.equal(a, b) for a, b in zip(keep, (ev._store.scores, ev._store.pred, ev._store.labels)))


def test_metrics_with_an_active_comm_is_refused():
    from mla_hip import Evaluator, JointEvaluator

    class Forced:                                            # a communicator that says it spans more than one rank
        active = True
    with pytest.raises(NotImplementedError, match="across ranks"):
        Evaluator(_clip_model(_ClipArgs), comm=Forced(), metrics=True, capacity=8)
    with pytest.raises(NotImplementedError, match="across ranks"):
        JointEvaluator(_clip_model(_JointClipArgs), comm=Forced(), metrics=True, capacity=8)


def test_joint_evaluator_store_agrees_with_its_counters():
    from mla_hip import JointEvaluator
    model, (tok, img, label) = _clip_model(_JointClipArgs), _clip_data()
    n = N_BATCHES * BATCH
    ev, twin = JointEvaluator(model, metrics=True, capacity=n + 1), JointEvaluator(model)
    assert twin._store is None and ev._store.H == 3
    for b in range(N_BATCHES):
        s = slice(b * BATCH, (b + 1) * BATCH)
        out, out_m = [t.clone() for t in ev.update(tok[s], img[s], label[s])]
        out_t, out_m_t = twin.update(tok[s], img[s], label[s])
        assert torch.equal(out, out_t) and torch.equal(out_m, out_m_t) and torch.equal(ev.counts, twin.counts)
    c = ev.counts.view(5, CLASSES).cpu().numpy()            # [num, argmax(out), out, out_a, out_v]
    conf = check_store_against_counters(ev, [c[1], c[3], c[4]], c[0], n)
    assert tuple(np.trace(k) / n for k in conf) == ev.result()
    ev.reset()
    assert ev.scores[3] == 0


def test_qmf_evaluator_store_agrees_with_its_counters():
    from mla_hip import AVClassifier, QMFEvaluator, attach_qmf_heads
    n, C = N_BATCHES * BATCH, CLASSES
    model = AVClassifier(_AVArgs(), seed=0)
    heads = attach_qmf_heads(model, seed=4)
    with torch.no_grad():
        for h in heads:
            h.weight.mul_(3.0)
    feats = [O.portable_normal(3, (n, 512), stream=60 + m).cuda() for m in range(2)]
    label = O.portable_labels(3, n, C).cuda()
    ev, twin = QMFEvaluator(model, metrics=True, capacity=n + 2), QMFEvaluator(model)
    assert twin._store is None and ev._store.H == 3
    for b in range(N_BATCHES):
        s = slice(b * BATCH, (b + 1) * BATCH)
        model.forward_raw = lambda *a: [f[s].contiguous() for f in feats]    # the encoders are not what is counted here
        out, z = [t.clone() for t in ev.update(None, None, label[s])]
        out_t, z_t = twin.update(None, None, label[s])
        assert torch.equal(out, out_t) and torch.equal(z, z_t) and torch.equal(ev.counts, twin.counts)
    c = ev.counts.view(5, C).cpu().numpy()
    conf = check_store_against_counters(ev, [c[1], c[3], c[4]], c[0], n)
    assert tuple(np.trace(k) / n for k in conf) == ev.result()


def test_rows_the_per_sample_kernel_counts_nowhere_are_stored_without_a_class():
    """gate_absent with alphas (1, 0, 0): a row whose only share of the fusion is absent is counted nowhere by mla_eval_head (pred -1,
    NaN fused row).  The store keeps such a row as a row without a class, so confusion() still sums to the counters."""
    import eval_model as E
    import test_eval_head_gpu as TE
    from mla_hip import Evaluator
    M, B, C = 3, 64, 4
    outs, label = E.sample_dense_case(M, B, C)
    present = E.every_pattern(B)
    al = (1.0, 0.0, 0.0)
    m = E.eval_rows(outs, label, 0, al, present=present)
    assert 0 < m.bad.sum() < B
    ev = Evaluator(TE.StubModal3(C), gate_absent=True, a_alpha=al[0], v_alpha=al[1], t_alpha=al[2], metrics=True, capacity=B + 1)
    ev.update(*[dev(o) for o in outs], dev(label, torch.int64), present=torch.from_numpy(present))
    pc = ev.per_class()
    assert (pc == m.counts).all() and pc[0].sum() == B - m.bad.sum()
    scores, pred, labels, n = ev.scores
    stored = labels.cpu().numpy()
    assert n == B and (stored[m.bad] == -1).all() and (stored[~m.bad] == label[~m.bad]).all()
    conf = ev.confusion()
    for h in range(1 + M):
        assert (np.diag(conf[h]) == pc[1 + h]).all() and (conf[h].sum(axis=1) == pc[0]).all()
