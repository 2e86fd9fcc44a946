"""csrc/gate_sweep.hip on the GPU: mla_gate_sweep, the gated fusion w_m ~ a_m exp(-beta H_m) of one batch at every gate of a grid in one
launch, and mla_eval_head_gated, one batch under one gate.

  1. exact, saturated      every row holds one logit far above integer logits on a coarse lattice: H = 0 exactly, so every gate
                           collapses to its prior (multiples of 2^-8 that sum to 1) at every beta and the tables are
                           sweep_model.sweep's on the priors, bit for bit; every mapping remainder (second softmax slot, second tile
                           of gates, the row-tile stride loop, the largest grid) and every row tile
  2. cross-kernel          dense logits: the unit gate against mla_eval_head mode 1, beta = 0 against mla_fusion_sweep, the apply
                           call against its gate's sweep row, all bit for bit.  mla_eval_head keeps its entropies to itself, so
                           ent_out is pinned by what they imply: the unit gate's weights ARE mode 1's, the apply call predicts
                           what the sweep predicts at every gate, ent_out has the same bits at every grid size and row tile, and
                           lies within fp32 rounding of the fp64 entropy
  3. dense against fp64    tests/gate_model.py on the grid of eight betas; a pair is compared where its fp64 top-two margin stands
                           clear of M (1 + beta) WEIGHT_TOL max|logit| (tests/test_gate_sweep_cpu.py holds the inputs to that)
  4. policies, refusals, Evaluator(gate_sweep= / gate_prior= / gate_beta=)
"""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_model as EM  # noqa: E402
import gate_model as GM  # noqa: E402
import sweep_model as SM  # noqa: E402
import test_eval_head_gpu as TH  # noqa: E402
from test_sweep_gpu import Tables, same_tables  # noqa: E402

F32, F64 = np.float32, np.float64
dev, bits, same_bits, Arena = TH.dev, TH.bits, TH.same_bits, TH.Arena
PEAK = 1024.0                    # 512 above the lattice's largest logit: exp(-512) is exactly 0 in fp32


@pytest.fixture(scope="module")
def ops():
    from mla_hip import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def run_sweep(ops, outs, labels, grid, present=None, tables=None, rows=slice(None), ent=True):
    """One ops.gate_sweep call on guarded tables -> (tables, ent_out (rows, M) host or None)."""
    outs = np.asarray(outs, dtype=F32)
    M, B, C = outs.shape
    t = tables or Tables(grid.shape[0], C)
    ar = Arena()
    n = len(range(B)[rows])
    e = ar.f32(n, M, name="ent_out") if ent else None
    ops.gate_sweep([dev(outs[m][rows]) for m in range(M)], dev(np.asarray(labels)[rows], torch.int64), dev(np.asarray(grid, dtype=F32)),
                   t.tp, t.pp, num=t.num, present=None if present is None else dev(np.asarray(present)[rows], torch.uint8), ent_out=e)
    ar.check()
    return t, (e.cpu().numpy() if ent else None)


def run_gated(ops, outs, labels, prior, beta, present=None, counts=None):
    """ops.eval_head_gated through the identity head on guarded outputs."""
    M, (B, C) = len(outs), outs[0].shape
    W, b = EM.identity_head(C)
    ar = Arena()
    logits, fused, weights = ar.f32(M, B, C, name="logits_out"), ar.f32(B, C, name="fused_out"), ar.f32(B, M, name="weights_out")
    pred = ar.i32(B, 1 + M, name="pred_out")
    if counts is None:
        counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    ops.eval_head_gated([dev(np.asarray(o, dtype=F32)) for o in outs], dev(W), dev(b), dev(np.asarray(labels), torch.int64), counts, logits,
                        prior=[float(v) for v in prior], beta=float(beta), present=None if present is None else dev(present, torch.uint8),
                        fused_out=fused, weights_out=weights, pred_out=pred)
    ar.check()
    for m in range(M):
        same_bits(logits[m].cpu().numpy(), np.asarray(outs[m], dtype=F32), f"identity head: logits_out[{m}]")
    return SimpleNamespace(fused=fused.cpu().numpy(), weights=weights.cpu().numpy(), pred=pred.cpu().numpy().astype(np.int64),
                           counts=counts.view(2 + M, C).cpu().numpy().astype(np.int64), counts_dev=counts)


def tables_of_pred(pred0, labels, C, present=None):
    """(tp (C), pp (C)) a fused prediction column (B,), -1 where the row made none, implies."""
    labels = np.asarray(labels)
    made = pred0 >= 0
    return np.bincount(labels[made & (pred0 == labels)], minlength=C), np.bincount(pred0[made], minlength=C)


# ---- 1. exact, saturated -------------------------------------------------------------------------------------------------------------
EXACT = [(2, 1, 2, 1), (3, 7, 65, 257), (2, 600, 6, 3), (3, 5, 128, 4096)]


def saturated_case(M, B, C, G):
    outs, labels, _ = SM.exact_case(M, B, C, G, seed=77 * M + B + C + G)
    rng = np.random.default_rng(M + B + C + G)
    at = rng.integers(0, C, size=(M, B))
    for m in range(M):
        outs[m, np.arange(B), at[m]] = PEAK
    parts = rng.integers(0, 257, size=(G, M))
    if M == 2:
        parts[:, 1] = 256 - parts[:, 0]
    else:
        parts[:, 1] = (parts[:, 1] * (256 - parts[:, 0])) // 256
        parts[:, 2] = 256 - parts[:, 0] - parts[:, 1]
    priors = (parts / 256).astype(F32)
    assert (priors.astype(F64).sum(axis=1) == 1).all() and priors.min() >= 0
    return outs, labels, priors


@pytest.mark.parametrize("M,B,C,G", EXACT)
def test_saturated_rows_collapse_every_gate_to_its_prior_bit_for_bit(ops, M, B, C, G):
    outs, labels, priors = saturated_case(M, B, C, G)
    assert (GM.entropies(outs, F32) == 0).all()
    want = SM.sweep(outs, labels, priors)
    fs = Tables(G, C)
    ops.fusion_sweep([dev(o) for o in outs], dev(labels, torch.int64), dev(priors), fs.tp, fs.pp, num=fs.num)
    same_tables(fs.host(), want, "mla_fusion_sweep on the priors")
    try:
        for tile in (1, 2, 4) if B > 1 else (1,):
            assert ops.gate_sweep_tile(tile) == tile
            for beta in (0, 1, 16):
                grid = np.concatenate([priors, np.full((G, 1), beta, dtype=F32)], axis=1)
                t, ent = run_sweep(ops, outs, labels, grid)
                same_tables(t.host(), want, f"M={M} B={B} C={C} G={G} beta={beta} tile={tile}")
                assert (bits(ent) == 0).all()                                # +0.0, not -0.0
    finally:
        assert ops.gate_sweep_tile(1) == 1


# ---- 2. cross-kernel, bit for bit ------------------------------------------------------------------------------------------------------
def lattice_priors(M):
    if M == 2:
        return np.array([(k / 256, 1 - k / 256) for k in range(257)], dtype=F32)
    return np.array([(i / 256, j / 256, (256 - i - j) / 256) for i in range(0, 257, 16) for j in range(0, 257 - i, 16)], dtype=F32)


def six_gates(M):
    rows = [[1.0] * M + [1.0], [0.55, 0.45, 0.3][:M] + [16.0], [0.0] + [1.0] * (M - 1) + [2.0], [0.0] * M + [2.0],
            [1024.0, 0.25, 3.0][:M] + [0.5], [0.7, 0.0, 0.3][:M] + [0.0]]
    return np.array(rows, dtype=F32)


@pytest.mark.parametrize("M,B,C", GM.DENSE_SHAPES)
def test_dense_logits_agree_with_eval_head_fusion_sweep_and_the_apply_call(ops, M, B, C):
    outs, labels = EM.sample_dense_case(M, B, C)
    outs = [np.asarray(o, dtype=F32) for o in outs]
    H64 = GM.entropies(outs)
    pri = lattice_priors(M)
    gates = six_gates(M)
    grid = np.concatenate([np.ones((1, M + 1), dtype=F32), np.concatenate([pri, np.zeros((len(pri), 1), dtype=F32)], axis=1), gates])
    g_gates = 1 + len(pri)
    ents = []
    for present in (None, EM.every_pattern(B, M)):
        name = f"(M, B, C) = {(M, B, C)}, present {'given' if present is not None else 'None'}"
        t, ent = run_sweep(ops, outs, labels, grid, present)
        tp, pp, num = t.host()
        ents.append(ent)
        if present is None:
            tp_all, pp_all = tp, pp
        # the unit gate is mla_eval_head mode 1
        head = TH.through_identity(ops, outs, labels, 1, [0.0] * M, present=present)
        want_tp, want_pp = tables_of_pred(head.pred[:, 0], labels, C)
        assert (tp[0] == want_tp).all() and (pp[0] == want_pp).all() and (num == head.counts[0]).all(), name
        unit = run_gated(ops, outs, labels, [1.0] * M, 1.0, present)
        same_bits(unit.weights, head.weights, name + ": weights of the unit gate")
        same_bits(unit.fused, head.fused, name + ": fused row of the unit gate")
        assert (unit.pred == head.pred).all() and (unit.counts == head.counts).all()
        # beta = 0 with priors that sum to 1 is mla_fusion_sweep
        fs = Tables(len(pri), C)
        ops.fusion_sweep([dev(o) for o in outs], dev(labels, torch.int64), dev(pri), fs.tp, fs.pp, num=fs.num,
                         present=None if present is None else dev(present, torch.uint8))
        ftp, fpp, fnum = fs.host()
        assert (tp[1:g_gates] == ftp).all() and (pp[1:g_gates] == fpp).all() and (num == fnum).all(), name
        # the apply call and its gate's sweep row
        left_out = 0
        for i, gate in enumerate(gates):
            got = run_gated(ops, outs, labels, gate[:M], gate[M], present)
            g = g_gates + i
            want_tp, want_pp = tables_of_pred(got.pred[:, 0], labels, C)
            assert (tp[g] == want_tp).all() and (pp[g] == want_pp).all() and (tp[g] == got.counts[1]).all(), (name, gate)
            bad = got.pred[:, 0] < 0
            left_out += int(bad.sum())
            assert (got.counts[0] == np.bincount(labels[~bad], minlength=C)).all() and num.sum() - pp[g].sum() == bad.sum()
            assert np.isnan(got.weights[bad]).all() and np.isnan(got.fused[bad]).all() and (got.pred[bad] == -1).all()
            assert np.isfinite(got.weights[~bad]).all() and (np.abs(got.weights[~bad].astype(F64).sum(axis=1) - 1) <= 1e-6).all()
            if present is not None:
                assert (bits(got.weights[~bad])[present[~bad] == 0] == 0).all()
        assert left_out >= B                                                 # the all-zero prior leaves every row out
    # ent_out: the same bits whatever is present, at every grid size and row tile; fp32 rounding away from the fp64 entropy
    same_bits(ents[0], ents[1], "ent_out with and without present")
    try:
        for tile, rows in ((1, slice(0, 1)), (2, slice(None)), (4, slice(None))):
            ops.gate_sweep_tile(tile)
            sub = grid[:1] if tile == 2 else grid
            t, ent = run_sweep(ops, outs, labels, sub, rows=rows)
            same_bits(ent, ents[0][rows], f"ent_out at tile {tile}")
            if tile != 1:
                got = t.host()
                assert (got[0] == tp_all[:len(sub)]).all() and (got[1] == pp_all[:len(sub)]).all()
    finally:
        assert ops.gate_sweep_tile(1) == 1
    err = float(np.abs(ents[0].astype(F64) - H64).max())
    print(f"(M, B, C) = {(M, B, C)}: ent_out off the fp64 entropy by {err:.3g} (tol {EM.WEIGHT_TOL:g})")
    assert err <= EM.WEIGHT_TOL          # H <= ln 128 = 4.85: a dozen fp32 roundings of that size are 3e-6


def test_torch_ops_are_the_same_launches(ops):
    M, B, C = 3, 9, 6
    outs, labels = EM.sample_dense_case(M, B, C)
    outs = [np.asarray(o, dtype=F32) for o in outs]
    grid, present = six_gates(M), EM.every_pattern(B, M)
    t, ent = run_sweep(ops, outs, labels, grid, present)
    u = Tables(len(grid), C)
    e = torch.empty((B, M), device="cuda")
    torch.ops.mla_hip.gate_sweep(dev(np.stack(outs)), dev(labels, torch.int64), dev(grid), u.tp, u.pp, u.num, dev(present, torch.uint8), e)
    same_tables(u.host(), t.host(), "torch op")
    same_bits(e.cpu().numpy(), ent, "torch op: ent_out")
    W, b = EM.identity_head(C)
    want = run_gated(ops, outs, labels, grid[1, :M], grid[1, M], present)
    counts = torch.zeros(C * (2 + M), device="cuda", dtype=torch.int32)
    logits, fused, weights, pred = torch.ops.mla_hip.eval_head_gated([dev(o) for o in outs], dev(W), dev(b), dev(labels, torch.int64), counts,
                                                                     [float(v) for v in grid[1, :M]], float(grid[1, M]), dev(present, torch.uint8))
    same_bits(weights.cpu().numpy(), want.weights, "torch op: weights")
    same_bits(fused.cpu().numpy(), want.fused, "torch op: fused")
    assert (pred.cpu().numpy() == want.pred).all() and torch.equal(counts, want.counts_dev)


# ---- 3. dense against fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,C", GM.DENSE_SHAPES)
def test_dense_grid_predicts_the_fp64_model_wherever_the_margin_is_clear(ops, M, B, C):
    outs, labels, grid, model, compared = GM.dense_case(M, B, C)
    G = grid.shape[0]
    share = 1 - compared.mean()
    assert share <= GM.UNCOMPARED_CAP
    # pair by pair: one launch per row on a pp table of its own; the one count of a table row is that pair's prediction
    per_row = torch.zeros((B, G, C), device="cuda", dtype=torch.int32)
    scratch = torch.zeros((G, C), device="cuda", dtype=torch.int32)
    d_outs, d_lab, d_grid = [dev(o) for o in outs], dev(labels, torch.int64), dev(grid)
    for r in range(B):
        ops.gate_sweep([o[r:r + 1] for o in d_outs], d_lab[r:r + 1], d_grid, scratch, per_row[r])
    pr = per_row.cpu().numpy()
    assert (pr.sum(axis=2) == 1).all()                                       # priors that sum to 1: no pair is left out
    pred = pr.argmax(axis=2).T                                               # (G, B)
    wrong = compared & (pred != model.pred)
    print(f"(M, B, C) = {(M, B, C)}: {G} gates, {share:.4%} of the pairs uncompared, {int(wrong.sum())} compared pairs off the model, "
          f"{int((~compared & (pred != model.pred)).sum())} uncompared ones")
    assert not wrong.any(), np.argwhere(wrong)[:5]
    t, _ = run_sweep(ops, outs, labels, grid, ent=False)                     # the one launch counts what the B launches predicted
    want = SM.count_tables(pred, labels, C)
    same_tables(t.host(), want, "one launch against one launch per row")
    # the apply call at one gate per beta
    n_prior = G // len(GM.DENSE_BETAS)
    scale = M * max(float(np.abs(o).max()) for o in outs)
    for i in range(len(GM.DENSE_BETAS)):
        g = i * n_prior + (7 * i + 3) % n_prior
        beta = float(grid[g, M])
        got = run_gated(ops, list(outs), labels, grid[g, :M], beta)
        assert (got.pred[:, 0] == pred[g]).all()                             # what the sweep predicts, near ties included
        tol = (1 + beta) * EM.WEIGHT_TOL
        dw = float(np.abs(got.weights.astype(F64) - model.w[g]).max())
        df = float(np.abs(got.fused.astype(F64) - model.fused[g]).max())
        print(f"  gate {grid[g].tolist()}: weights off by {dw:.3g} (tol {tol:.3g}), fused off by {df:.3g} (tol {tol * scale:.3g})")
        assert dw <= tol and df <= tol * scale


# ---- 4. policies -----------------------------------------------------------------------------------------------------------------------
def policy_case():
    """130 rows of pure saturated rows (H = 0, the peaks of a row's modalities on different classes), every presence pattern, labels
    -1 and C among them: a pair predicts the peak of its eligible modality with the largest prior, whatever the rounding."""
    M, B, C = 3, 130, 5
    outs = np.stack([np.stack([EM.saturated_row(C, (r + m) % C) for r in range(B)]) for m in range(M)])
    present = EM.every_pattern(B)
    rng = np.random.default_rng(5)
    labels = np.array([(r + rng.integers(0, M)) % C for r in range(B)], dtype=np.int64)
    labels[3], labels[40], labels[129] = -1, C, 2 ** 40
    grid = np.array([[0, 0.5, 0.25, 1], [0.5, 0, 0.25, 16], [0.5, 0.25, 0, 0], [0, 0, 1, 2], [0, 0, 0, 1], [0.3, 0.2, 0.5, 4], [3, 2, 1, 0.5]],
                    dtype=F32)
    return outs, labels, grid, present


def test_policies_left_out_pairs_bad_labels_accumulation_split_and_rerun(ops):
    outs, labels, grid, present = policy_case()
    M, B, C = outs.shape
    want = GM.sweep(outs, labels, grid, present, dtype=F32)
    assert all((a == b).all() for a, b in zip(want, GM.sweep(outs, labels, grid, present)))
    t, _ = run_sweep(ops, outs, labels, grid, present)
    got = t.host()
    same_tables(got, want, "policies")
    tp, pp, num = got
    counted = SM.row_counted(labels, C, present)
    assert num.sum() == counted.sum() == B - 3 and (num == np.bincount(labels[counted], minlength=C)).all()
    # a zero prior on everything a row has: left out of tp / pp, still in num
    for g in range(len(grid)):
        has_share = ((present != 0) & (grid[g, :M] > 0)[None]).any(axis=1)
        assert pp[g].sum() == (counted & has_share).sum(), g
    assert pp[4].sum() == 0 and tp[4].sum() == 0 and (pp[[5, 6]].sum(axis=1) == num.sum()).all() and (pp[:4].sum(axis=1) < num.sum()).all()
    # two calls accumulate; the tables do not depend on the batch split; a rerun gives the same bits
    twice, _ = run_sweep(ops, outs, labels, grid, present, tables=t)
    same_tables(twice.host(), tuple(2 * w for w in want), "two calls")
    d_outs, d_labels, d_grid, d_present = GM.dense_case(3, 130, 128)[0], GM.dense_case(3, 130, 128)[1], GM.dense_grid(3), EM.every_pattern(130)
    whole, ent = run_sweep(ops, d_outs, d_labels, d_grid, d_present)
    whole = whole.host()
    again, ent2 = run_sweep(ops, d_outs, d_labels, d_grid, d_present)
    same_tables(again.host(), whole, "rerun")
    same_bits(ent2, ent, "rerun: ent_out")
    halves, e0 = run_sweep(ops, d_outs, d_labels, d_grid, d_present, rows=slice(0, 64))
    _, e1 = run_sweep(ops, d_outs, d_labels, d_grid, d_present, tables=halves, rows=slice(64, 130))
    same_tables(halves.host(), whole, "64 + 66")
    same_bits(np.concatenate([e0, e1]), ent, "64 + 66: ent_out")
    ones = Tables(d_grid.shape[0], 128)
    for r in range(130):
        run_sweep(ops, d_outs, d_labels, d_grid, d_present, tables=ones, rows=slice(r, r + 1), ent=False)
    same_tables(ones.host(), whole, "1 x 130")


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,match", [("M1", "need M = 2 or 3"), ("M4", "need M = 2 or 3"), ("C129", "need 0 < C <= 128"),
                                        ("G0", r"need 0 < G <= 4096 gates \(got 0\)"), ("G4097", r"need 0 < G <= 4096 gates \(got 4097\)"),
                                        ("null_tp", "null pointer"), ("labels_off", "8-byte")])
def test_sweep_refusals_launch_nothing(what, match):
    from mla_hip import _lib
    lib = _lib.load()
    M = {"M1": 1, "M4": 4}.get(what, 2)
    B, C, G = 5, (129 if what == "C129" else 6), {"G0": 0, "G4097": 4097}.get(what, 8)
    ar = Arena()
    tp, pp, num, ent = ar.i32(4097, C, name="tp"), ar.i32(4097, C, name="pp"), ar.i32(C, name="num"), ar.f32(B, 4, name="ent_out")
    l = [torch.zeros((B, C), device="cuda") for _ in range(3)]
    labels = torch.zeros(B + 1, device="cuda", dtype=torch.int64)
    grid = torch.ones((4097, 5), device="cuda")
    rc = lib.mla_gate_sweep(l[0].data_ptr(), l[1].data_ptr(), l[2].data_ptr(), labels.data_ptr() + (4 if what == "labels_off" else 0), None,
                            grid.data_ptr(), None if what == "null_tp" else tp.data_ptr(), pp.data_ptr(), num.data_ptr(), ent.data_ptr(),
                            M, B, C, G, None)
    assert rc == -1
    assert re.search(match, lib.mla_last_error().decode()) and "mla_gate_sweep" in lib.mla_last_error().decode()
    ar.check(written=False)


@pytest.mark.parametrize("what,match", [("nan_prior", "need a finite prior0"), ("inf_beta", "need a finite beta"), ("neg_prior", "need a finite prior1"),
                                        ("neg_beta", "need a finite beta"), ("prior_cap", r"prior0 in \[0, 1024\]"), ("beta_cap", r"beta in \[0, 16\]"),
                                        ("M4", "need M = 2 or 3"), ("C129", "need 0 < C <= 128"), ("null", "null pointer")])
def test_apply_refusals_launch_nothing(ops, what, match):
    from mla_hip._lib import MLAHipError
    M, B, D = 2, 5, 64
    C = 129 if what == "C129" else 6
    prior = {"nan_prior": [float("nan"), 1.0], "neg_prior": [1.0, -1e-3], "prior_cap": [1024.5, 1.0]}.get(what, [0.55, 0.45])
    beta = {"inf_beta": float("inf"), "neg_beta": -0.5, "beta_cap": 16.5}.get(what, 2.0)
    n = 4 if what == "M4" else M
    ar = Arena()
    logits, fused, weights, pred = ar.f32(n, B, C), ar.f32(B, C), ar.f32(B, n), ar.i32(B, 1 + n)
    counts = ar.i32(C * (2 + n))
    feats = [torch.zeros((B, D), device="cuda") for _ in range(n)]
    with pytest.raises(MLAHipError, match=match):
        ops.eval_head_gated(feats, torch.zeros((C, D), device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(B, device="cuda", dtype=torch.int64),
                            counts, None if what == "null" else logits, prior=prior + [1.0] * (n - M), beta=beta, fused_out=fused,
                            weights_out=weights, pred_out=pred)
    ar.check(written=False)


# ---- 6. through Evaluator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dynamic,mode", [(False, "batch"), (True, "batch"), (True, "sample")])
def test_evaluator_gate_sweep_leaves_the_evaluation_untouched_and_its_best_gate_can_be_applied(ops, monkeypatch, dynamic, mode):
    from mla_hip import Evaluator, gate_grid
    model, (tok, img, label), B = TH._clip_model(), TH._clip_data(), 10
    tok, img, label = tok.cuda(), img.cuda(), label.cuda()
    n = 2 * B
    grid = gate_grid(2)
    kw = dict(dynamic=dynamic, dynamic_mode=mode, av_alpha=0.55)
    ev, twin = Evaluator(model, gate_sweep=grid, **kw), Evaluator(model, **kw)
    assert twin._gate_sweep is None
    launches = []
    real = ops.gate_sweep
    monkeypatch.setattr(ops, "gate_sweep", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    for k, s in enumerate((slice(0, B), slice(B, n))):
        outs = [o.clone() for o in ev.update(tok[s], img[s], label[s])]
        outs_twin = twin.update(tok[s], img[s], label[s])
        assert len(launches) == k + 1                        # ONE launch per update, none without gate_sweep=
        assert all(torch.equal(a, c) for a, c in zip(outs, outs_twin))
        assert torch.equal(ev.counts, twin.counts) and torch.equal(ev.weights, twin.weights)
        if ev.per_sample:
            assert torch.equal(ev.fused, twin.fused) and torch.equal(ev.pred, twin.pred) and torch.equal(ev.sample_weights, twin.sample_weights)
    assert ev.result() == twin.result() and (ev.per_class() == twin.per_class()).all()
    s, pc = ev.gate_sweep_result(), ev.per_class()
    assert (s.num == pc[0]).all() and s.num.sum() == n and s.counted.max() == n
    at = 11                                                  # beta = 0, priors (0.55, 1.0 - 0.55): the fixed fusion of av_alpha = 0.55
    assert s.beta[at] == 0 and s.priors[at].tolist() == [float(F32(0.55)), float(F32(1.0 - 0.55))]
    if not dynamic:
        assert (s.tp[at] == pc[1]).all() and s.acc[at] == ev.result()[0]
    prior, beta, value, g = s.best("acc")
    assert value == s.acc.max() and g == int(np.flatnonzero(s.acc == s.acc.max())[0]) and (prior == grid[g, :2].numpy()).all() and beta == float(grid[g, 2])
    # the gate the search found, applied: the counters of its sweep row
    for gg in (g, 2 * 21 + 11, 5 * 21 + 20):                 # ... and (0.55, 0.45, beta = 1), (1, 0, beta = 8)
        ap = Evaluator(model, dynamic=True, dynamic_mode="sample", gate_prior=s.priors[gg], gate_beta=float(s.beta[gg]), metrics=True, capacity=n)
        for sl in (slice(0, B), slice(B, n)):
            ap.update(tok[sl], img[sl], label[sl])
        assert (ap.per_class()[1] == s.tp[gg]).all() and (ap.per_class()[0] == s.num).all(), gg
        conf = ap.confusion()[0]
        assert (np.diag(conf) == s.tp[gg]).all() and (conf.sum(axis=0) == s.pp[gg]).all()
        assert ap.f1("macro")[0] == s.f1("macro")[gg]
    ev.reset()
    z = ev.gate_sweep_result()
    assert z.tp.sum() == 0 and z.pp.sum() == 0 and z.num.sum() == 0 and ev.per_class().sum() == 0
    ev.update(tok[:B], img[:B], label[:B])
    assert ev.gate_sweep_result().num.sum() == B
    with pytest.raises(ValueError, match="dynamic_mode='sample'"):
        Evaluator(model, dynamic=dynamic and mode == "batch", gate_prior=prior)


def test_evaluator_unit_gate_is_the_sample_mode_and_one_sided_gates_default_to_one():
    from mla_hip import Evaluator
    model, (tok, img, label) = TH._clip_model(), TH._clip_data()
    tok, img, label = tok.cuda(), img.cuda(), label.cuda()
    plain = Evaluator(model, dynamic=True, dynamic_mode="sample")
    plain.update(tok, img, label)
    keep = [t.clone() for t in (plain.sample_weights, plain.fused, plain.pred, plain.counts)]
    for kw in (dict(gate_beta=1), dict(gate_prior=[1, 1]), dict(gate_prior=[1, 1], gate_beta=1.0)):
        ev = Evaluator(model, dynamic=True, dynamic_mode="sample", **kw)
        ev.update(tok, img, label)
        assert all(torch.equal(a, b) for a, b in zip(keep, (ev.sample_weights, ev.fused, ev.pred, ev.counts))), kw
    sharp = Evaluator(model, dynamic=True, dynamic_mode="sample", gate_beta=8)
    sharp.update(tok, img, label)
    w, w1 = sharp.sample_weights.cpu().numpy(), keep[0].cpu().numpy()
    assert (np.abs(w - 0.5) >= np.abs(w1 - 0.5)).all() and (np.abs(w - 0.5) > np.abs(w1 - 0.5)).any()      # sharper, row by row


@pytest.mark.parametrize("metrics", [False, True])
def test_evaluator_gate_absent_takes_the_present_matrix_into_the_gate_sweep_and_the_applied_gate(metrics):
    from mla_hip import Evaluator, gate_grid
    M, B, C = 3, 64, 4
    outs, label = EM.sample_dense_case(M, B, C)
    present = EM.every_pattern(B)
    grid = torch.cat([gate_grid(3, betas=(0, 2), steps=4), torch.tensor([[1, 1, 1, 1], [0.35, 0.25, 0.4, 0]], dtype=torch.float32)])
    unit, fixed = grid.shape[0] - 2, grid.shape[0] - 1
    feats, lab, have = [dev(np.asarray(o, dtype=F32)) for o in outs], dev(label, torch.int64), torch.from_numpy(present)
    evs = {"sample": Evaluator(TH.StubModal3(C), dynamic=True, dynamic_mode="sample", gate_absent=True, gate_sweep=grid),
           "fixed": Evaluator(TH.StubModal3(C), gate_absent=True, gate_sweep=grid)}
    for ev in evs.values():
        for s in (slice(0, 30), slice(30, B)):
            ev.update(*[f[s] for f in feats], lab[s], present=have[s])
    s = evs["sample"].gate_sweep_result()
    z = evs["fixed"].gate_sweep_result()
    assert all((a == b).all() for a, b in zip((s.tp, s.pp, s.num), (z.tp, z.pp, z.num)))       # the sweep does not depend on the evaluator's mode
    assert (s.tp[unit] == evs["sample"].per_class()[1]).all() and (s.num == evs["sample"].per_class()[0]).all() and s.num.sum() == B
    # beta = 0 at the evaluator's alphas renormalises over what a row has as the fixed path does (in fp64 instead of fp32: the margins
    # of these rows stand clear of that, eval_model.EVAL_MARGIN in test_eval_head_gpu.py)
    assert (s.tp[fixed] == evs["fixed"].per_class()[1]).all()
    assert (s.counted[[unit, fixed]] == B).all() and (s.counted < B).any()                     # lattice rows with a zero leave pairs out
    g = int(np.flatnonzero(s.counted < B)[-1])                                                 # a gate that leaves pairs out, applied
    ap = Evaluator(TH.StubModal3(C), dynamic=True, dynamic_mode="sample", gate_absent=True, gate_prior=s.priors[g], gate_beta=float(s.beta[g]),
                   metrics=metrics, capacity=B if metrics else None)
    ap.update(*feats, lab, present=have)
    pc = ap.per_class()
    assert (pc[1] == s.tp[g]).all() and pc[0].sum() == s.counted[g] and int((ap.pred[:, 0] < 0).sum()) == B - s.counted[g]
    w = ap.sample_weights.cpu().numpy()
    made = (ap.pred[:, 0] >= 0).cpu().numpy()
    assert np.isnan(w[~made]).all() and (bits(w[made])[present[made] == 0] == 0).all()
    if metrics:
        conf = ap.confusion()[0]
        assert (np.diag(conf) == s.tp[g]).all() and (conf.sum(axis=0) == s.pp[g]).all() and conf.sum() == s.counted[g]
    # without gate_absent the masks are ignored by the evaluator's fusion, and so by its gate sweep
    ev = Evaluator(TH.StubModal3(C), dynamic=True, dynamic_mode="sample", gate_sweep=grid)
    ev.update(*feats, lab, present=have)
    s = ev.gate_sweep_result()
    assert (s.counted[:-2][grid[:-2, :3].sum(dim=1).numpy() > 0] == B).all() and (s.tp[unit] == ev.per_class()[1]).all()
