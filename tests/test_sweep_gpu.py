"""csrc/fusion_sweep.hip on the GPU: the fixed-weight fusion of one batch at every row of a grid of fusion weights, in one launch.

  1. exact (bit for bit)   exactly-summable inputs (integer logits with many ties, weights that are multiples of 2^-8) against the
                           restatement of tests/sweep_model.py, at every value of each axis and the tile remainders of the mapping
                           (SWEEP_LANES = 256 grid points per workgroup, row tiles striding past 256 workgroups: B = 257); guards stay poisoned; two calls
                           accumulate to the concatenated batch's tables
  2. the parent's kernels  dense fp32 logits: tp[g] against mla_eval_fuse's fused-correct counter and tp[g] / pp[g] against the
                           predictions of mla_eval_head (mode 0) with alphas = grid[g], with and without missing modalities
  3. the near tie          a batch on which the fused and the unfused rounding of sum_m w_m l_m predict different classes in every
                           row: the sweep predicts what mla_eval_fuse and mla_eval_head predict
  4. Evaluator(sweep=)     the grid row equal to the evaluator's own alphas reproduces its counters, on both of its paths
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sweep_model as SM  # noqa: E402

F32 = np.float32
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


class Tables:
    """tp (G, C), pp (G, C), num (C): zeroed int32 tables inside poisoned guards."""

    def __init__(self, G, C):
        self.flats = []
        self.tp, self.pp, self.num = self._new(G, C), self._new(G, C), self._new(C)

    def _new(self, *shape):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * GUARD,), IFILL, dtype=torch.int32, device="cuda")
        flat[GUARD:GUARD + n] = 0
        self.flats.append((flat, n))
        return flat[GUARD:GUARD + n].view(shape)

    def host(self):
        torch.cuda.synchronize()
        for flat, n in self.flats:
            assert bool((flat[:GUARD] == IFILL).all()) and bool((flat[GUARD + n:] == IFILL).all()), "a guard was overwritten"
        return tuple(t.cpu().numpy().astype(np.int64) for t in (self.tp, self.pp, self.num))


def run(ops, outs, labels, grid, present=None, tables=None, rows=slice(None)):
    M, B, C = outs.shape
    t = tables or Tables(grid.shape[0], C)
    ops.fusion_sweep([dev(outs[m][rows]) for m in range(M)], dev(labels[rows], torch.int64), dev(grid), t.tp, t.pp, num=t.num,
                     present=None if present is None else dev(present[rows], torch.uint8))
    return t


def same_tables(got, want, name):
    for g, w, which in zip(got, want, ("tp", "pp", "num")):
        assert g.shape == w.shape and (g == w).all(), f"{name}: {which} differs at {np.argwhere(g != w)[:5].tolist()}"


# ---- 1. exactly-summable inputs ------------------------------------------------------------------------------------------------------
# every M, every C in {1, 3, 6, 64, 65, 101, 128}, every B in {1, 7, 64, 65, 257} and every G
# in {1, 63, 64, 65, 256, 257, 861, 4096} (lane-tile remainders of 256) at least once, and the corners
EXACT = [(2, 1, 1, 1), (3, 3, 7, 63), (2, 6, 64, 64), (3, 64, 65, 65), (2, 65, 257, 256), (3, 101, 64, 257), (2, 128, 7, 861),
         (3, 3, 7, 4096), (2, 1, 257, 4096), (3, 128, 257, 1), (3, 128, 65, 4096), (2, 128, 257, 861), (3, 1, 1, 4096), (2, 128, 1, 1)]


def exact_inputs(M, C, B, G, flavour):
    outs, labels, grid = SM.exact_case(M, B, C, G, seed=1000 * M + 7 * C + B + G)
    present = None
    if flavour == "holes":                                   # bad labels and rows with nothing present; the others have everything,
        rng = np.random.default_rng(B + G)                   # so no weight is divided and every sum stays exact
        labels[rng.random(B) < 0.2] = -1
        labels[rng.random(B) < 0.1] = C
        labels[rng.random(B) < 0.1] = 2 ** 40
        present = np.ones((B, M), dtype=np.uint8)
        present[rng.random(B) < 0.25] = 0
    return outs, labels, grid, present


@pytest.mark.parametrize("flavour", ["plain", "holes"])
@pytest.mark.parametrize("M,C,B,G", EXACT)
def test_exact_inputs_equal_the_restatement_bit_for_bit(ops, M, C, B, G, flavour):
    outs, labels, grid, present = exact_inputs(M, C, B, G, flavour)
    pred = SM.predict(outs, labels, grid, present)
    assert (pred == SM.predict(outs, labels, grid, present, fused=True)).all()       # exact: no rounding to tell the forms apart
    want = SM.count_tables(pred, labels, C, present)
    got = run(ops, outs, labels, grid, present).host()
    same_tables(got, want, f"M={M} C={C} B={B} G={G} {flavour}")
    assert (got[1].sum(axis=1) == want[2].sum()).all()                               # nothing is left out here: every row predicts
    if G > 1:                                                                        # grid row 1 = (1, 0[, 0]): modality 0 alone
        ok = SM.row_counted(labels, C, present)
        assert (got[1][1] == np.bincount(outs[0].argmax(axis=1)[ok], minlength=C)).all()
    assert (got[1][0, 1:] == 0).all()                                                # grid row 0 = zeros: all ties, the first class
    if B >= 2:                                                                       # two calls, split at an odd row
        k = B // 2 + 1
        t = run(ops, outs, labels, grid, present, rows=slice(0, k))
        run(ops, outs, labels, grid, present, tables=t, rows=slice(k, B))
        same_tables(t.host(), want, f"M={M} C={C} B={B} G={G} {flavour}, two calls")


def test_num_is_optional_and_the_torch_op_is_the_same_launch(ops):
    M, C, B, G = 3, 6, 9, 65
    outs, labels, grid, present = exact_inputs(M, C, B, G, "holes")
    want = SM.sweep(outs, labels, grid, present)
    t = Tables(G, C)
    ops.fusion_sweep([dev(o) for o in outs], dev(labels, torch.int64), dev(grid), t.tp, t.pp, present=dev(present, torch.uint8))
    got = t.host()
    same_tables(got[:2], want[:2], "num=None")
    assert (got[2] == 0).all()
    t = Tables(G, C)
    torch.ops.mla_hip.fusion_sweep(dev(outs), dev(labels, torch.int64), dev(grid), t.tp, t.pp, t.num, dev(present, torch.uint8))
    same_tables(t.host(), want, "torch op")


# ---- 2. the parent's kernels on dense inputs -----------------------------------------------------------------------------------------
def dense_grid(M):
    rng = np.random.default_rng(40 + M)
    if M == 2:
        rows = [(0.55, 1.0 - 0.55), (0.5, 0.5), (1, 0), (0, 1), (0, 0), (0.3, 0.7), (0.05, 0.95)]
    else:
        rows = [(0.35, 0.25, 0.4), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0.5, 0.5), (0.5, 0, 0.5), (0.5, 0.5, 0), (0, 0, 0)]
    rows += [tuple(r) for r in rng.random((12 - len(rows), M))]
    return np.array(rows, dtype=np.float64).astype(F32)


def head_case(M, B, C, D=64):
    rng = np.random.default_rng(100 * M + C)
    feats = rng.standard_normal((M, B, D)).astype(F32)
    W = (rng.standard_normal((C, D)) * 0.2).astype(F32)
    b = (rng.standard_normal(C) * 0.1).astype(F32)
    labels = rng.integers(0, C, size=B).astype(np.int64)
    return feats, W, b, labels


def present_kinds(M, B):
    rng = np.random.default_rng(7 * M + B)
    keep = (rng.random((B, M)) < 0.6).astype(np.uint8)
    some_empty = keep.copy()
    keep[np.arange(B), rng.integers(0, M, size=B)] = 1       # every row keeps a modality
    some_empty[::5] = 0
    only_one = np.zeros((B, M), dtype=np.uint8)              # a single modality per row: the one-hot and zero grid rows give it no share
    only_one[np.arange(B), np.arange(B) % M] = 1
    return {"all": None, "kept": keep, "some_empty": some_empty, "only_one": only_one}


def eval_head_rows(ops, feats, W, b, labels, alphas, present):
    """(logits (M, B, C) device, pred (B,) host): mla_eval_head, mode 0; pred -1 where it counted the row nowhere."""
    M, B, _ = feats.shape
    C = W.shape[0]
    logits = torch.empty((M, B, C), device="cuda", dtype=torch.float32)
    pred = torch.empty((B, 1 + M), device="cuda", dtype=torch.int32)
    counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    ops.eval_head([dev(f) for f in feats], dev(W), dev(b), dev(labels, torch.int64), counts, logits, mode=0,
                  alphas=[float(a) for a in alphas], present=None if present is None else dev(present, torch.uint8), pred_out=pred)
    return logits, pred[:, 0].cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("C", [6, 101])
@pytest.mark.parametrize("M", [2, 3])
def test_dense_inputs_agree_with_eval_fuse_and_eval_head_for_every_grid_row(ops, M, C):
    B = 64
    feats, W, b, labels = head_case(M, B, C)
    grid = dense_grid(M)
    assert grid.shape == (12, M)
    for kind, P in present_kinds(M, B).items():
        logits = None
        preds = np.empty((12, B), dtype=np.int64)
        for g in range(12):
            logits, preds[g], counts = eval_head_rows(ops, feats, W, b, labels, grid[g], P)
            if P is None:                                    # mla_eval_fuse on the same logits: its fused-correct counter
                fuse_counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
                ops.eval_fuse([logits[m] for m in range(M)], dev(labels, torch.int64), fuse_counts, None, False, [float(a) for a in grid[g]])
                fc = fuse_counts.cpu().numpy()
                assert (fc[C:2 * C] == counts[C:2 * C]).all()
                preds_fuse_tp = fc[C:2 * C]
            else:
                preds_fuse_tp = None
            if g == 0:
                t = Tables(12, C)
                ops.fusion_sweep([logits[m] for m in range(M)], dev(labels, torch.int64), dev(grid), t.tp, t.pp, num=t.num,
                                 present=None if P is None else dev(P, torch.uint8))
                tp, pp, num = t.host()
            if preds_fuse_tp is not None:
                assert (tp[g] == preds_fuse_tp).all(), (kind, g)
        counted = SM.row_counted(labels, C, P)
        assert (num == np.bincount(labels[counted], minlength=C)).all(), kind
        for g in range(12):
            made = preds[g] >= 0
            assert not made[~counted].any()
            assert (pp[g] == np.bincount(preds[g][made], minlength=C)).all(), (kind, g)
            assert (tp[g] == np.bincount(labels[made & (preds[g] == labels)], minlength=C)).all(), (kind, g)
        left_out = counted[None] & (preds < 0)               # eval_head's -1 on a countable row: the eligible alphas sum to nothing
        if kind in ("all", "kept"):
            assert left_out.any() == (kind == "kept")        # the zero grid row with every modality fuses to +0.0 (class 0) ...
        if kind == "only_one":
            assert left_out.sum() >= B                       # ... renormalising what is left of it is what leaves a pair out
            # pair by pair: one launch per row on tables of its own; the pairs without a prediction are exactly eval_head's -1
            per_row = torch.zeros((B, 12, C), device="cuda", dtype=torch.int32)
            scratch = torch.zeros((12, C), device="cuda", dtype=torch.int32)
            Pd, lab = dev(P, torch.uint8), dev(labels, torch.int64)
            d_grid = dev(grid)
            for r in range(B):
                ops.fusion_sweep([logits[m][r:r + 1] for m in range(M)], lab[r:r + 1], d_grid, scratch, per_row[r], present=Pd[r:r + 1])
            made_dev = per_row.sum(dim=2).cpu().numpy().T    # (12, B): 1 where the pair predicted
            assert ((made_dev == 1) == (preds >= 0)).all() and set(np.unique(made_dev)) <= {0, 1}


# ---- 3. the near tie -----------------------------------------------------------------------------------------------------------------
def near_tie_rows(C=8):
    """Rows of the construction in the module docstring of the CPU test: A = (-1, 1 + 2^-12), B = (2^-11 + 2^-25, 0) under the grid row
    (1, 1 + 2^-12), A and B at varying indices, scaled by powers of two, among classes far below."""
    e = F32(2.0 ** -12)
    rows, labels = [], []
    for ia in range(C):
        for ib in range(C):
            if ia == ib:
                continue
            scale = F32(2.0 ** ((ia * C + ib) % 13 - 6))
            row = np.full((2, C), -100.0, dtype=F32) * scale
            row[:, ia] = np.array([-1, F32(1) + e], dtype=F32) * scale
            row[:, ib] = np.array([F32(2.0 ** -11 + 2.0 ** -25), 0], dtype=F32) * scale
            rows.append(row)
            labels.append(ia if (ia + ib) % 2 else ib)
    outs = np.ascontiguousarray(np.stack(rows, axis=1))      # (2, B, C)
    return outs, np.array(labels, dtype=np.int64), np.array([[1, F32(1) + e]], dtype=F32)


def test_near_ties_follow_the_rounding_of_the_evaluators_kernels(ops):
    outs, labels, grid = near_tie_rows()
    M, B, C = outs.shape
    plain, fused = SM.predict(outs, labels, grid)[0], SM.predict(outs, labels, grid, fused=True)[0]
    assert (plain != fused).all()                            # the two restatement forms disagree on every row
    assert ((plain == labels) != (fused == labels)).all()    # ... and exactly one of them is the label
    # mla_eval_head forms its logits from features: an identity head hands the rows through exactly (x * 1 and zeros)
    W, b = np.eye(C, dtype=F32), np.zeros(C, dtype=F32)
    logits, head_pred, head_counts = eval_head_rows(ops, outs, W, b, labels, grid[0], None)
    assert torch.equal(logits.cpu(), torch.from_numpy(outs))
    fuse_counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    d_outs, d_lab = [dev(o) for o in outs], dev(labels, torch.int64)
    ops.eval_fuse(d_outs, d_lab, fuse_counts, None, False, [float(a) for a in grid[0]])
    fuse_tp = fuse_counts.cpu().numpy()[C:2 * C]
    form = {True: "fused", False: "unfused"}[bool((head_pred == fused).all())]
    print(f"near ties: mla_eval_head follows the {form} form")
    assert (head_pred == (fused if form == "fused" else plain)).all()
    assert (fuse_tp == head_counts[C:2 * C]).all()           # the two parent kernels agree with each other
    # the sweep, alone and among other grid rows (another lane, another tile of lanes)
    for G, at in ((1, 0), (300, 0), (300, 299), (300, 255), (300, 256)):
        big = np.tile(np.array([[0.5, 0.5]], dtype=F32), (G, 1))
        big[at] = grid[0]
        tp, pp, num = run(ops, outs, labels, big).host()
        assert (pp[at] == np.bincount(head_pred, minlength=C)).all(), (G, at)
        assert (tp[at] == np.bincount(labels[head_pred == labels], minlength=C)).all() and (tp[at] == fuse_tp).all(), (G, at)
        want = SM.count_tables((fused if form == "fused" else plain)[None], labels, C)
        assert (tp[at] == want[0][0]).all() and (pp[at] == want[1][0]).all() and (num == want[2]).all()
    print(f"near ties: mla_fusion_sweep follows the {form} form on {B} rows")


# ---- 4. through Evaluator ------------------------------------------------------------------------------------------------------------
class _ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


BATCHES, DIM, CLASSES = (10, 10, 7), 64, 6                  # three batches, the last one short


def _clip_model():
    from mla_hip import CLIPClassifier
    model = CLIPClassifier(_ClipArgs(), seed=3, feat_dim=DIM)
    rng = np.random.default_rng(11)
    with torch.no_grad():                                    # a head that separates the classes: logits of order 1
        head = model.fusion_module.fc_out
        head.weight.copy_(torch.from_numpy((rng.standard_normal(tuple(head.weight.shape)) * 0.2).astype(F32)))
        head.bias.copy_(torch.from_numpy((rng.standard_normal(tuple(head.bias.shape)) * 0.1).astype(F32)))
    return model


def _clip_data():
    rng = np.random.default_rng(12)
    n = sum(BATCHES)
    tok, img = (torch.from_numpy(rng.standard_normal((n, 1, DIM)).astype(F32)).cuda() for _ in range(2))
    return tok, img, torch.from_numpy(rng.integers(0, CLASSES, size=n)).cuda()


def _batches():
    at = 0
    for b in BATCHES:
        yield slice(at, at + b)
        at += b


@pytest.mark.parametrize("dynamic,mode,metrics", [(False, "batch", False), (False, "batch", True), (True, "batch", False),
                                                  (True, "sample", False), (True, "sample", True)])
def test_evaluator_sweep_reproduces_its_counters_and_sweep_none_is_unchanged(ops, monkeypatch, dynamic, mode, metrics):
    from mla_hip import Evaluator, fusion_grid
    model, (tok, img, label) = _clip_model(), _clip_data()
    n = sum(BATCHES)
    grid = fusion_grid(2, 20)
    at = 11                                                  # row 11 = (0.55, 1.0 - 0.55): the evaluator's own alphas
    assert grid[at].tolist() == [float(F32(0.55)), float(F32(1.0 - 0.55))]
    kw = dict(dynamic=dynamic, dynamic_mode=mode, av_alpha=0.55)
    ev = Evaluator(model, sweep=grid, metrics=metrics, capacity=n if metrics else None, **kw)
    twin = Evaluator(model, **kw)
    assert twin._sweep is None
    launches = []
    real = ops.fusion_sweep
    monkeypatch.setattr(ops, "fusion_sweep", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    for k, s in enumerate(_batches()):
        outs = [o.clone() for o in ev.update(tok[s], img[s], label[s])]
        assert len(launches) == k + 1                        # ONE launch per update ...
        outs_twin = twin.update(tok[s], img[s], label[s])
        assert len(launches) == k + 1                        # ... and none without sweep=
        assert all(torch.equal(a, c) for a, c in zip(outs, outs_twin))
        assert torch.equal(ev.counts, twin.counts) and torch.equal(ev.weights, twin.weights)
        if ev.per_sample:
            assert torch.equal(ev.fused, twin.fused) and torch.equal(ev.pred, twin.pred)
    assert ev.result() == twin.result() and (ev.per_class() == twin.per_class()).all()
    s, pc = ev.sweep_result(), ev.per_class()
    assert (s.num == pc[0]).all() and s.num.sum() == n and (s.counted == n).all()
    assert (s.tp[0] == pc[3]).all() and (s.tp[20] == pc[2]).all()          # (0, 1) is modality 1 alone, (1, 0) modality 0
    if not dynamic:                                          # the evaluator's own fusion is the fixed one of grid row 11
        assert (s.tp[at] == pc[1]).all() and s.acc[at] == ev.result()[0]
        if metrics:
            assert (np.diag(ev.confusion()[0]) == s.tp[at]).all() and (ev.confusion()[0].sum(axis=0) == s.pp[at]).all()
            assert s.f1("macro")[at] == ev.f1("macro")[0] and s.f1("weighted")[at] == ev.f1("weighted")[0]
    w, value, g = s.best("acc")
    assert value == s.acc.max() and value >= s.acc[at] and (w == grid[g].numpy()).all()
    ev.reset()                                               # restarts
    z = ev.sweep_result()
    assert z.tp.sum() == 0 and z.pp.sum() == 0 and z.num.sum() == 0
    first = next(_batches())
    ev.update(tok[first], img[first], label[first])
    again = ev.sweep_result()
    assert again.num.sum() == BATCHES[0] and (again.num == ev.per_class()[0]).all()
    bad = label[first].clone()                               # labels that are no class change no table
    bad[:3] = torch.tensor([-1, CLASSES, 2 ** 40], device="cuda")
    keep = [t.clone() for t in (ev._sweep.tp, ev._sweep.pp, ev._sweep.num)]
    ev.update(tok[first][:3], img[first][:3], bad[:3])
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(keep, (ev._sweep.tp, ev._sweep.pp, ev._sweep.num)))


class StubModal3:
    """What Evaluator asks of a three-modality model whose forward takes present=: the features are handed in directly, in
    mla_encoders() order (a, v, t), under a dense shared head."""

    def __init__(self, C, D):
        from mla_hip.model import SharedHead
        self.device = torch.device("cuda")
        self.fusion_module = SimpleNamespace(fc_out=SharedHead(D, C, "cuda", seed=0))
        rng = np.random.default_rng(21)
        with torch.no_grad():
            self.fusion_module.fc_out.weight.copy_(torch.from_numpy((rng.standard_normal((C, D)) * 0.2).astype(F32)))
            self.fusion_module.fc_out.bias.copy_(torch.from_numpy((rng.standard_normal(C) * 0.1).astype(F32)))

    def mla_encoders(self):
        return [("a", "audio", None), ("v", "image", None), ("t", "text", None)]

    def forward_raw(self, *inputs, present=None):
        return tuple(inputs)

    def eval(self):
        return self


@pytest.mark.parametrize("metrics", [False, True])
def test_evaluator_gate_absent_sweep_takes_the_same_present_matrix(metrics):
    from mla_hip import Evaluator, fusion_grid
    C, D = 4, 64
    rng = np.random.default_rng(31)
    n = sum(BATCHES)
    feats = [torch.from_numpy(rng.standard_normal((n, D)).astype(F32)).cuda() for _ in range(3)]
    label = torch.from_numpy(rng.integers(0, C, size=n)).cuda()
    have = (rng.random((n, 3)) < 0.5).astype(np.uint8)
    have[np.arange(n), rng.integers(0, 3, size=n)] = 1       # the evaluator refuses a row with nothing present
    present = torch.from_numpy(have)
    assert bool((present.sum(dim=1) == 1).any()) and bool((present.sum(dim=1) == 3).any())
    grid = torch.cat([fusion_grid(3, 4), torch.tensor([[0.35, 0.25, 0.4]], dtype=torch.float64).to(torch.float32)])
    at = grid.shape[0] - 1                                   # the evaluator's own (default) alphas
    ev = Evaluator(StubModal3(C, D), gate_absent=True, sweep=grid, metrics=metrics, capacity=n if metrics else None)
    twin = Evaluator(StubModal3(C, D), gate_absent=True)
    for s in _batches():
        ev.update(*[f[s] for f in feats], label[s], present=present[s])
        twin.update(*[f[s] for f in feats], label[s], present=present[s])
        assert torch.equal(ev.counts, twin.counts) and torch.equal(ev.pred, twin.pred) and torch.equal(ev.fused, twin.fused)
    s, pc = ev.sweep_result(), ev.per_class()
    assert (s.num == pc[0]).all() and s.num.sum() == n
    assert (s.tp[at] == pc[1]).all() and s.counted[at] == s.num.sum()
    assert (s.counted[:at] <= s.num.sum()).all() and (s.counted[:at] < s.num.sum()).any()        # lattice rows with a zero leave pairs out
    if metrics:
        conf = ev.confusion()[0]
        assert (np.diag(conf) == s.tp[at]).all() and (conf.sum(axis=0) == s.pp[at]).all() and (conf.sum(axis=1) == s.num).all()
        assert s.f1("macro")[at] == ev.f1("macro")[0]
    # without gate_absent the evaluator's own fusion ignores the masks, and so does its sweep
    ev = Evaluator(StubModal3(C, D), sweep=grid)
    for s in _batches():
        ev.update(*[f[s] for f in feats], label[s], present=present[s])
    s, pc = ev.sweep_result(), ev.per_class()
    assert (s.num == pc[0]).all() and s.num.sum() == n and (s.counted == n).all() and (s.tp[at] == pc[1]).all()
