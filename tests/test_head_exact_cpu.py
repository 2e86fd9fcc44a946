"""No GPU, no library: the inputs of tests/head_exact.py prove what test_head_exact_gpu.py says they prove.

  * the shape tables reach every regime of the head kernels' loops;
  * LIN and SAT are exact: the sum budgets hold (asserted where the inputs are built), the SAT margin is >= 128, both kinds of label
    occur at the rows where a row loop turns, and a plain float32 evaluation equals the fp64 one bit for bit;
  * UNI's float32 restatement has s = C exactly;
  * the fault table: every fault, restated in the model, changes the outputs of the class that is meant to prove it by at least one
    unit on EVERY table shape that reaches it;
  * DENSE: the cross-entropy families contain the spike class and another one as labels; the QMF cases keep every ranking decision
    of the fp64 model 1e-4 from its threshold and contain a duplicate index."""
import numpy as np
import pytest
import torch

import head_exact as H

F32, F64 = torch.float32, torch.float64
IDS = lambda s: "-".join(map(str, s))                                       # noqa: E731


def test_tables_reach_every_regime():
    for axis, values in ((0, (1, 3, 5, 64, 65, 130)), (1, (8, 63, 64, 65, 70, 256, 257, 320)), (2, (1, 2, 3, 17, 63, 64, 65, 127, 128))):
        seen = [s[axis] for s in H.TABLE]
        assert set(seen) == set(values), (axis, sorted(set(seen)))
        for v in values:
            assert seen.count(v) >= 2, f"axis {axis}: {v} occurs {seen.count(v)} times"
    assert len(set(H.TABLE)) == len(H.TABLE) and 20 <= len(H.TABLE) <= 28
    meets = lambda **kw: any(all(s["BDC".index(k)] == v for k, v in kw.items()) for s in H.TABLE)      # noqa: E731
    assert meets(B=130, D=257) and meets(B=130, C=128) and meets(D=257, C=128)
    for v in (129, 200, 257):                                               # third and fifth 64-trip of the general loops
        assert [s[2] for s in H.WIDE].count(v) >= 2
    assert {s[0] for s in H.WIDE} >= {1, 3, 5, 64, 65, 130}
    md = {(M, D) for M, (_, D, _) in zip(H.MODS, H.TABLE)}
    assert {(3, 70), (2, 320), (3, 257)} <= md and {M for M, _ in md} == {2, 3}
    assert all(C <= 128 for _, _, C in H.TABLE)
    # every fault is reached by at least two table shapes
    for name, (reached, _, _) in H.FAULTS.items():
        shapes = H.WIDE if name == "ce_trip3" else H.TABLE
        n = sum(bool(reached(B, D, C, M, 0.5)) for M, (B, D, C) in zip(H.MODS * 2, shapes))
        assert n >= 2, name


@pytest.mark.parametrize("shape", H.TABLE + H.WIDE, ids=IDS)
def test_lin_is_exact_in_float32(shape):
    B, D, C = shape
    c = H.lin_case(B, D, C)                                                  # the budgets are asserted inside
    assert max(c.budget.values()) < 24
    assert torch.equal(H.logits_model(c.X, c.W, c.b, dt=F32).double(), H.logits_model(c.X, c.W, c.b))
    for scale in H.SCALES:
        w64, w32 = H.bwd_model(c.xs, c.W, c.dl, scale), H.bwd_model(c.xs, c.W, c.dl, scale, dt=F32)
        for a, b in zip((w64[0], w64[1], *w64[2]), (w32[0], w32[1], *w32[2])):
            assert torch.equal(b.double(), a)


@pytest.mark.parametrize("M,shape", list(zip(H.MODS, H.TABLE)), ids=lambda v: IDS(v) if isinstance(v, tuple) else str(v))
def test_lin_concat_is_exact_in_float32(M, shape):
    c = H.lin_case(*shape, M)
    assert (c.b == 0).all() == (M == 3)
    for a, b in zip(H.concat_fwd_model(c.xs, c.W, c.b), H.concat_fwd_model(c.xs, c.W, c.b, dt=F32)):
        assert torch.equal(b.double(), a)
    for scale in H.SCALES:
        w64, w32 = H.bwd_model(c.xs, c.W, c.dl, scale), H.bwd_model(c.xs, c.W, c.dl, scale, dt=F32)
        for a, b in zip((w64[0], w64[1], *w64[2]), (w32[0], w32[1], *w32[2])):
            assert torch.equal(b.double(), a)


@pytest.mark.parametrize("M,shape", [(1, s) for s in H.TABLE] + list(zip(H.MODS, H.TABLE)),
                         ids=lambda v: IDS(v) if isinstance(v, tuple) else str(v))
def test_sat_conditions(M, shape):
    B, D, C = shape
    c = H.sat_case(B, D, C, M)
    assert c.margin >= H.MARGIN, c.margin
    logits = H.logits_model(c.X, c.W, c.b)
    assert torch.equal(logits * 16, (logits * 16).round()), "logits off the 2^-4 grid"
    assert torch.equal(logits.argmax(1), c.win)
    # the code sits where a column loop turns
    cols = H.code_cols(D)
    assert 0 in cols and D - 1 in cols and all(v in cols for v in (63, 64, 255, 256) if v < D)
    # label mix at the rows where a row loop turns
    hit = c.labels == c.win
    rows = sorted({r for r in (0, 63, 64, B - 1) if r < B})
    if C > 1 and len(rows) > 1:
        assert hit[rows].any() and not hit[rows].all(), (rows, hit[rows])
        assert abs(hit.double().mean().item() - 1 / 3) < 0.34
    if C > 64:
        assert int(c.win[0]) >= 64                                           # a winner in the second softmax slot
    if B > 64 and C > 1:
        assert not hit[64:].all()                                            # a non-zero row loss past the first trip of head_col_sum
    # the saturated softmax: one-hot, exactly
    rowloss, dl, loss = H.ce_model(logits, c.labels, H.INV)
    assert set(torch.unique(dl).tolist()) <= {0.0, H.INV, -H.INV}
    want = (logits.max(1).values - logits[torch.arange(B), c.labels]) * H.INV
    assert torch.equal(rowloss, want) and torch.equal(loss, want.sum())
    # float32 = fp64, bit for bit
    if M == 1:
        a, b = H.feature_model(c.X, c.W, c.b, c.labels, H.INV, H.LR), H.feature_model(c.X, c.W, c.b, c.labels, H.INV, H.LR, dt=F32)
        h64, h32 = H.head_model(c.X, c.W, c.b, c.labels, H.INV), H.head_model(c.X, c.W, c.b, c.labels, H.INV, dt=F32)
        pairs = [(getattr(a, k), getattr(b, k)) for k in ("logits", "loss", "dl", "buf", "W", "b")] + [(h64.dX, h32.dX)]
    else:
        a, b = H.concat_model(c.xs, c.W, c.b, c.labels, H.INV), H.concat_model(c.xs, c.W, c.b, c.labels, H.INV, dt=F32)
        pairs = [(getattr(a, k), getattr(b, k)) for k in ("out", "out_m", "dl", "loss", "dW", "db")] + list(zip(a.dxs, b.dxs))
    for x64, x32 in pairs:
        assert x32.dtype == F32 and torch.equal(x32.double(), x64)


@pytest.mark.parametrize("shape", H.TABLE, ids=IDS)
def test_sat_bad_labels_zero_their_rows(shape):
    B, D, C = shape
    c = H.sat_case(B, D, C)
    bad = H.with_bad_labels(c.labels, C)
    g, w = H.head_model(c.X, c.W, c.b, c.labels, H.INV), H.head_model(c.X, c.W, c.b, bad, H.INV)
    assert torch.isnan(w.loss) and torch.equal(w.logits, g.logits)
    keep = torch.ones(B, dtype=torch.bool)
    keep[0] = keep[-1] = False
    assert torch.equal(w.dl, g.dl * keep[:, None]) and (w.dl[~keep] == 0).all()


@pytest.mark.parametrize("shape", H.TABLE + H.WIDE, ids=IDS)
def test_uni_restatement(shape):
    B, D, C = shape
    c = H.uni_case(B, D, C)
    logits = H.logits_model(c.X, c.W, c.b, dt=F32)
    assert torch.equal(logits, c.logits)
    rowloss, dl, loss = H.ce_model(logits, c.labels, H.INV, dt=F32)
    p = torch.tensor(1.0, dtype=F32) / torch.tensor(float(C), dtype=F32)     # one correctly rounded division
    onehot = torch.nn.functional.one_hot(c.labels, C).float()
    assert dl.dtype == F32 and torch.equal(dl, (p - onehot) * torch.tensor(H.INV, dtype=F32))
    assert abs(loss.item() - B * np.log(C) * H.INV) <= 2e-6 + 2e-6 * B * np.log(C) * H.INV


def _case(cls, B, D, C, M):
    return {"LIN": H.lin_case, "SAT": H.sat_case}[cls](B, D, C, M) if cls != "UNI" else H.uni_case(B, D, C)


def _fault_cases():
    out = []
    for name, (reached, cls, _) in H.FAULTS.items():
        shapes = H.WIDE if name == "ce_trip3" else H.TABLE
        mods = [1] * len(shapes) if name != "concat_mod256" else H.MODS
        extra = list(zip(H.MODS, shapes)) if name in ("partial_block", "no_scale") else []
        for M, (B, D, C) in list(zip(mods, shapes)) + extra:
            for scale in H.SCALES if name == "no_scale" else (1.0,):
                if reached(B, D, C, M, scale):
                    out.append((name, cls, M, B, D, C, scale))
    return out


@pytest.mark.parametrize("name,cls,M,B,D,C,scale", _fault_cases(), ids=lambda v: str(v))
def test_fault_is_caught_on_every_shape_that_reaches_it(name, cls, M, B, D, C, scale):
    c = _case(cls, B, D, C, M)
    if name in ("colsum_64", "colsum_stride63"):
        good, bad = H.bwd_model(c.xs, c.W, c.dl)[1], H.bwd_model(c.xs, c.W, c.dl, fault=name)[1]
        assert ((good - bad).abs() >= 2.0 ** -6).all(), "db: every column must move"
        s = H.sat_case(B, D, C)                                              # and the loss sum
        if C > 1 and name == "colsum_64":
            assert H.differs(H.head_model(s.X, s.W, s.b, s.labels, H.INV).loss, H.head_model(s.X, s.W, s.b, s.labels, H.INV, fault=name).loss,
                             2.0 ** -11)
    elif name == "lane_tail":
        assert H.differs(H.logits_model(c.X, c.W, c.b), H.logits_model(c.X, c.W, c.b, fault=name), 2.0 ** -4)
    elif name in ("slot2_sum", "ce_trip3"):
        good, bad = H.ce_model(c.logits, c.labels, H.INV, dt=F32)[1], H.ce_model(c.logits, c.labels, H.INV, fault=name, dt=F32)[1]
        assert H.differs(good, bad, 2.0 ** -31)
        assert not torch.equal(good[:, :64], bad[:, :64])                    # in the classes every variant writes, too
    elif name == "slot2_max":
        good, bad = H.head_model(c.X, c.W, c.b, c.labels, H.INV), H.head_model(c.X, c.W, c.b, c.labels, H.INV, fault=name)
        assert H.differs(good.dl, bad.dl, H.INV) and H.differs(good.dW, bad.dW, H.INV / 4)
    else:                                                                    # partial_block, concat_mod256, no_scale
        good, bad = H.bwd_model(c.xs, c.W, c.dl, scale), H.bwd_model(c.xs, c.W, c.dl, scale, fault=name)
        assert H.differs(good[0], bad[0], 2.0 ** -9), "dW"
        assert H.differs(torch.cat(good[2], 1), torch.cat(bad[2], 1), 2.0 ** -9), "dx"
        if name == "no_scale":
            assert H.differs(good[1], bad[1], 2.0 ** -7), "db"


@pytest.mark.parametrize("family", H.CE_FAMILIES)
def test_dense_ce_labels(family):
    for B, C in {(B, C) for B, _, C in H.TABLE + H.WIDE}:
        c = H.dense_ce_case(B, C, family)
        assert c.logits.shape == (B, C) and c.logits.dtype == F32 and torch.isfinite(c.logits).all()
        assert int(c.labels.min()) >= 0 and int(c.labels.max()) < C
        if family == "spike":
            assert (c.logits.max(1).values > 5e3).all()
        if family == "low":
            assert (c.logits < -9e3).all()
        if B > 1 and C > 1:
            assert (c.labels == c.top).any() and (c.labels != c.top).any()


@pytest.mark.parametrize("family", H.CE_FAMILIES)
def test_dense_ce_loss_bound_is_within_reach_of_float32(family):
    """The loss bound of the GPU test, 2e-6 sum |row loss| + 2e-6, on a float32 evaluation of the model's own expression
    log(s) - (l[label] - max): kept with room.  ((max + log(s)) - l[label] in float32 misses it by two orders in `low`.)"""
    for B, C in {(B, C) for B, _, C in H.TABLE + H.WIDE}:
        c = H.dense_ce_case(B, C, family)
        rowloss, _, _ = H.ce_model(c.logits, c.labels, 1.0 / B)
        got = H.ce_model(c.logits, c.labels, 1.0 / B, dt=F32)[0].double().sum().item()
        assert abs(got - rowloss.sum().item()) <= 0.5 * (2e-6 * rowloss.abs().sum().item() + 2e-6), (B, C)


@pytest.mark.parametrize("shape", H.QMF_DENSE, ids=IDS)
def test_qmf_dense_conditions(shape):
    c = H.qmf_dense_case(*shape)
    assert len(c.steps) == 2
    seen_t = set()
    for st in c.steps:
        idx = st.idx.tolist()
        assert len(set(idx)) < len(idx), "no duplicate index in the batch"
        assert 0 <= min(idx) and max(idx) < c.n_data
        mg, ha, t = H.qmf_decisions(st.ref)
        assert torch.isfinite(mg).all() and torch.isfinite(ha).all()
        assert (mg[mg != 0] > H.QMF_DECISION).all() and (ha[t != 0].abs() > H.QMF_DECISION).all()
        assert (mg[t == 0] == 0).all()
        seen_t |= set(t.reshape(-1).tolist())
    assert {-1.0, 1.0} <= seen_t
