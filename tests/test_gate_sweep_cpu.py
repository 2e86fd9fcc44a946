"""CPU: the restatement of the gated fusion family (tests/gate_model.py) against the two rules it contains, gate_grid, the contract on
a gate and its overflow caps, the near-tie condition of the dense GPU comparison, the refusals of the additive ABI entries
mla_gate_sweep / mla_eval_head_gated (nothing is dereferenced before validation), `make host-check`, and Evaluator's gate_sweep= /
gate_prior= / gate_beta= argument rules."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import eval_model as EM
import gate_model as GM
import sweep_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_unit_gate_is_the_per_sample_entropy_gating():
    """a = 1, beta = 1: eval_model.row_weights(mode=1), on every presence pattern."""
    for M, B, C in [(2, 32, 6), (3, 65, 101), (3, 7, 128)]:
        outs, labels = EM.sample_dense_case(M, B, C)
        have = EM.every_pattern(B, M)
        grid = np.ones((1, M + 1))
        p = GM.pairs(outs, labels, grid, have)
        for r in range(B):
            rows = [o[r] for o in outs]
            want = EM.row_weights(rows, 1, None, have[r])
            w, ok = GM.row_weights(rows, grid[0, :M], 1.0, have[r])
            assert ok and (w == want).all() and (p.w[0, r] == want).all(), (M, B, C, r)
            assert w[have[r] == 0].tolist() == [0.0] * int((have[r] == 0).sum())
            w32, ok32 = GM.row_weights(rows, grid[0, :M], 1.0, have[r], dtype=F32)
            want32 = EM.row_weights(rows, 1, None, have[r], dtype=F32)   # sums g in fp32, the rule in fp64: an ulp of the sum apart
            assert ok32 and w32.dtype == F32 and np.abs(w32 - want32).max() <= 2.0 ** -23


def test_beta_zero_is_the_fixed_weight_fusion():
    """beta = 0 with priors (k / 256, 1 - k / 256): sweep_model.pair_weights, weight for weight, left-out pairs included; on exact
    inputs the tables are sweep_model.sweep's."""
    M, B, C = 2, 21, 7
    outs, labels, _ = SM.exact_case(M, B, C, 4, seed=3)
    priors = np.array([(k / 256, 1 - k / 256) for k in range(257)], dtype=F32)
    grid = np.concatenate([priors, np.zeros((257, 1), dtype=F32)], axis=1)
    have = EM.every_pattern(B, M)
    for present in (None, have):
        for dtype in (F32, F64):
            p = GM.pairs(outs, labels, grid, present, dtype=dtype)
            w, ok = SM.pair_weights(priors, B, present)
            assert (p.ok == ok).all() and (p.w[ok] == w[ok].astype(dtype)).all()
        assert not ok.all() or present is None                           # (0, 1) and (1, 0) leave single-modality rows out
        got, want = GM.sweep(outs, labels, grid, present, dtype=F32), SM.sweep(outs, labels, priors, present)
        assert all((g == w).all() for g, w in zip(got, want))
    # any beta: saturated rows have H = 0 exactly in fp32 (exp(-200) is 0 there), so every gate collapses to its prior
    sat = np.stack([np.stack([EM.saturated_row(C, (r + m) % C) for r in range(B)]) for m in range(M)])
    assert (GM.entropies(sat, F32) == 0).all() and GM.entropies(sat, F64).max() < 1e-80
    for beta in (1, 16):
        grid[:, M] = beta
        assert all((g == w).all() for g, w in zip(GM.sweep(sat, labels, grid, have, dtype=F32), SM.sweep(sat, labels, priors, have)))


def test_left_out_pairs_and_uncounted_rows_follow_the_sweep_policies():
    M, C = 3, 4
    outs = np.zeros((M, 6, C), dtype=F32)
    outs[0, :, 1] = 1
    outs[1, :, 2] = 1
    outs[2, :, 3] = 1
    labels = np.array([1, -1, C, 2 ** 40, 2, 3], dtype=np.int64)
    present = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 1, 0]], dtype=np.uint8)
    grid = np.array([[1, 0, 0, 2], [0, 1, 0, 0], [0.25, 0.25, 0.5, 16]], dtype=F32)
    p = GM.pairs(outs, labels, grid, present)
    # row 5 has only modality 1: the gate whose prior on it is zero is left out, the others give it everything
    assert p.pred.tolist() == [[1, -1, -1, -1, -1, -1], [2, -1, -1, -1, -1, 2], [3, -1, -1, -1, -1, 2]]
    assert p.ok[:, 5].tolist() == [False, True, True] and p.w[2, 5].tolist() == [0.0, 1.0, 0.0]
    tp, pp, num = GM.sweep(outs, labels, grid, present)
    assert num.tolist() == [0, 1, 0, 1] and pp.sum(axis=1).tolist() == [1, 2, 2] and tp.tolist() == [[0, 1, 0, 0], [0] * 4, [0] * 4]


# ---- gate_grid -----------------------------------------------------------------------------------------------------------------------
def test_gate_grid_is_beta_outer_fusion_grid_inner():
    from mla_hip import fusion_grid, gate_grid
    g = gate_grid(2, betas=(0, 0.5, 1, 2, 4, 8), steps=20)
    assert g.dtype == torch.float32 and tuple(g.shape) == (6 * 21, 3) and not g.is_cuda and g.is_contiguous()
    assert tuple(gate_grid(2).shape) == (126, 3) and torch.equal(gate_grid(2), g)
    inner = fusion_grid(2, 20)
    for i, beta in enumerate((0, 0.5, 1, 2, 4, 8)):
        blk = g[21 * i:21 * (i + 1)]
        assert torch.equal(blk[:, :2], inner) and (blk[:, 2] == beta).all()
    g3 = gate_grid(3, betas=(16, 0.25), steps=8)
    assert tuple(g3.shape) == (2 * 45, 4) and torch.equal(g3[:45, :3], fusion_grid(3, 8)) and torch.equal(g3[45:, :3], fusion_grid(3, 8))
    assert (g3[:45, 3] == 16).all() and (g3[45:, 3] == 0.25).all()                  # the order given, not sorted
    assert tuple(GM.dense_grid(2).shape) == (8 * 21, 3) and tuple(GM.dense_grid(3).shape) == (8 * 45, 4)
    with pytest.raises(ValueError, match="2 or 3"):
        gate_grid(4)
    with pytest.raises(ValueError, match="steps"):
        gate_grid(2, steps=0)
    with pytest.raises(ValueError, match="betas"):
        gate_grid(2, betas=())


# ---- the contract on a gate ----------------------------------------------------------------------------------------------------------
def test_the_caps_keep_every_intermediate_finite_in_fp32_at_128_classes():
    """The largest entropy gap is ln 128 (a uniform row against a saturated one): at beta = 16 and a = 1024 neither g_k nor the
    three-term sum overflows, and one step past either cap is what the contract keeps out."""
    from mla_hip.gate import GATE_MAX_BETA, GATE_MAX_PRIOR
    C = 128
    rows = [np.zeros(C, dtype=F32), EM.saturated_row(C, 5), EM.saturated_row(C, 9)]
    H = np.array([EM.row_entropy(r, F32) for r in rows], dtype=F32)
    assert H.dtype == F32 and abs(float(H[0]) - np.log(128)) < 1e-5 and H[1] == 0 and H[2] == 0
    x = F32(GATE_MAX_BETA) * (H.max() - H)
    assert x.dtype == F32 and float(x.max()) < 77.7 < float(np.log(np.finfo(F32).max))
    g = F32(GATE_MAX_PRIOR) * np.exp(x)
    assert g.dtype == F32 and np.isfinite(g).all() and float(g.max()) < 6e36
    s = F32(g.astype(F64).sum())
    assert np.isfinite(s) and s > 0
    w, ok = GM.row_weights(rows, [GATE_MAX_PRIOR] * 3, GATE_MAX_BETA, [1, 1, 1], dtype=F32)
    assert ok and np.isfinite(w).all() and abs(float(w.sum()) - 1) < 1e-6 and w[0] < 1e-30 and w[1] == w[2] == F32(0.5)
    p = GM.pairs(np.stack(rows)[:, None, :], [0], [[GATE_MAX_PRIOR] * 3 + [GATE_MAX_BETA]], dtype=F32)
    assert p.ok.all() and (p.w[0, 0] == w).all()
    with np.errstate(over="ignore"):                                                 # what the caps are for
        assert not np.isfinite(F32(GATE_MAX_PRIOR) * np.exp(F32(20) * (H.max() - H))).all()


# ---- the near-tie condition of the dense GPU comparison --------------------------------------------------------------------------------
def test_dense_cases_leave_at_most_one_percent_of_the_pairs_uncompared():
    """A condition on the inputs, on the fp64 model alone: the dense GPU test compares a pair only where the fp64 top-two margin of
    its fused row is at least M (1 + beta) WEIGHT_TOL max|logit|."""
    for M, B, C in GM.DENSE_SHAPES:
        outs, labels, grid, model, compared = GM.dense_case(M, B, C)
        assert model.ok.all() and (model.pred >= 0).all()                           # priors sum to 1 and everything is present
        share = 1 - compared.mean()
        print(f"gate sweep, dense (M, B, C) = {(M, B, C)}: {grid.shape[0]} gates, {share:.4%} of the pairs left uncompared")
        assert share <= GM.UNCOMPARED_CAP, (M, B, C, share)
        assert (GM.margin_floor(M, grid, outs)[grid[:, M] == 16] == M * 17.0 * EM.WEIGHT_TOL * float(np.abs(outs).max())).all()


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def test_abi_entries_are_additive_and_refuse_before_any_launch():
    from mla_hip import _lib, torch_ops
    lib = _lib.load()
    assert len(_lib.PROTOTYPES["mla_gate_sweep"][1]) == 15 and len(_lib.PROTOTYPES["mla_eval_head_gated"][1]) == 21
    assert lib.mla_abi_version() == 3                        # additive
    assert {"gate_sweep", "eval_head_gated"} <= set(torch_ops.op_names())
    fake = 0x1000                                            # non-null, aligned, never dereferenced: validation fails first
    err = lib.mla_last_error

    def sweep(l0=fake, l1=fake, l2=fake, labels=fake, present=None, grid=fake, tp=fake, pp=fake, num=None, ent=None, M=3, B=4, C=6, G=8):
        return lib.mla_gate_sweep(l0, l1, l2, labels, present, grid, tp, pp, num, ent, M, B, C, G, None)
    for M in (0, 1, 4, -2):
        assert sweep(M=M) == -1 and f"mla_gate_sweep: need M = 2 or 3 (got {M})".encode() in err()
    for null in ("l0", "l1", "l2", "labels", "grid", "tp", "pp"):
        assert sweep(**{null: None}) == -1 and b"mla_gate_sweep: null pointer" in err(), null
    for null in ("l0", "l1", "labels", "grid", "tp", "pp"):
        assert sweep(M=2, l2=None, **{null: None}) == -1 and b"mla_gate_sweep: null pointer" in err(), null
    for name in ("B", "C", "G"):
        for v in (0, -1):
            assert sweep(**{name: v}) == -1 and b"mla_gate_sweep: need" in err(), (name, v)
    assert sweep(C=129) == -1 and b"mla_gate_sweep: need 0 < C <= 128 (got 129)" in err()
    assert sweep(G=4097) == -1 and b"mla_gate_sweep: need 0 < G <= 4096 gates (got 4097)" in err()
    for off in ("l0", "l1", "l2", "grid", "tp", "pp", "num", "ent"):
        assert sweep(**{off: fake + 2}) == -1 and b"4-byte" in err(), off
    assert sweep(labels=fake + 4) == -1 and b"8-byte" in err()
    assert lib.mla_gate_sweep_tile(-1) == 1 and lib.mla_gate_sweep_tile(3) == 1      # the default tile; 3 is no tile: a query

    def head(x2=fake, counts=fake, M=3, B=4, D=8, C=6, prior=(1.0, 1.0, 1.0), beta=1.0, fused=None):
        return lib.mla_eval_head_gated(fake, fake, x2, fake, fake, fake, None, counts, fake, fused, None, None, M, B, D, C, *prior, beta, None)
    for M in (1, 4):
        assert head(M=M) == -1 and f"mla_eval_head_gated: need M = 2 or 3 (got {M})".encode() in err()
    assert head(x2=None) == -1 and b"mla_eval_head_gated: null pointer" in err()
    assert head(counts=None) == -1 and b"null pointer" in err()
    assert head(C=129) == -1 and b"mla_eval_head_gated: need 0 < C <= 128 (got 129)" in err()
    assert head(fused=fake + 2) == -1 and b"4-byte" in err()
    for prior in ((float("nan"), 1, 1), (1, float("inf"), 1), (1, 1, -0.25), (1025.0, 1, 1)):
        assert head(prior=prior) == -1 and b"mla_eval_head_gated: need a finite prior" in err(), prior
    for beta in (float("nan"), float("inf"), -1.0, 16.5):
        assert head(beta=beta) == -1 and b"mla_eval_head_gated: need a finite beta in [0, 16]" in err(), beta
    assert head(M=2, x2=None, prior=(1, 1, float("nan")), beta=-1.0) == -1 and b"beta" in err()      # prior2 is not read with M = 2
    with pytest.raises(Exception):                           # no CPU implementation: torch's "no kernel" error
        torch.ops.mla_hip.gate_sweep(torch.zeros(2, 4, 3), torch.zeros(4, dtype=torch.int64), torch.zeros(5, 3),
                                     torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int32))


def test_host_check_builds_and_runs_the_gate_program():
    csrc = os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "host-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gate host check ok" in r.stdout and "gate_host_check.cpp" in r.stdout and "-fsanitize=address,undefined" in r.stdout


# ---- Evaluator's argument rules ------------------------------------------------------------------------------------------------------
class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


def test_evaluator_takes_the_gate_arguments_and_defaults_to_nothing():
    from mla_hip import CLIPClassifier, Evaluator, GateSweep, GateSweepResult, gate_grid
    from mla_hip._lib import MLAHipError
    params = inspect.signature(Evaluator.__init__).parameters
    assert all(params[k].default is None for k in ("gate_sweep", "gate_prior", "gate_beta"))
    model = CLIPClassifier(ClipArgs(), device="cpu", seed=0, feat_dim=64)
    ev = Evaluator(model)
    assert ev._gate_sweep is None and ev._gate is None
    with pytest.raises(MLAHipError, match="gate_sweep=None"):
        ev.gate_sweep_result()
    ev.reset()                                               # nothing to zero
    grid = gate_grid(2)
    ev = Evaluator(model, gate_sweep=grid)                   # host tensors: nothing is launched before the first update
    sw = ev._gate_sweep
    assert isinstance(sw, GateSweep) and (sw.M, sw.C, sw.G) == (2, 6, 126) and ev._gate is None and ev._sweep is None
    assert sw.tp.shape == (126, 6) and sw.pp.shape == (126, 6) and sw.num.shape == (6,)
    assert sw.tp.dtype == sw.pp.dtype == sw.num.dtype == torch.int32 and torch.equal(sw.grid, grid)
    s = ev.gate_sweep_result()                               # empty tables answer zeros
    assert isinstance(s, GateSweepResult) and s.priors.dtype == F32 and s.priors.shape == (126, 2) and s.beta.shape == (126,)
    assert (s.priors == grid[:, :2].numpy()).all() and (s.beta == grid[:, 2].numpy()).all()
    assert s.tp.dtype == s.pp.dtype == s.num.dtype == s.counted.dtype == np.int64
    assert s.acc.tolist() == [0.0] * 126 and s.f1("macro").shape == (126,)
    prior, beta, value, g = s.best("acc")
    assert (g, value, beta) == (0, 0.0, 0.0) and (prior == s.priors[0]).all()
    with pytest.raises(ValueError, match="metric"):
        s.best("map")
    sw.tp += 1
    ev.reset()
    assert int(sw.tp.sum()) == 0
    # counting is SweepResult's: first maximum in grid order, left-out pairs are errors
    r = GateSweepResult(np.array([[.5, .5], [1, 0], [0, 1]], dtype=F32), np.array([0, 2, 2], dtype=F32), np.array([[1, 0], [2, 0], [2, 0]]),
                        np.array([[2, 1], [3, 0], [2, 0]]), np.array([2, 1]))
    assert r.acc.tolist() == [1 / 3, 2 / 3, 2 / 3] and r.counted.tolist() == [3, 3, 2]
    prior, beta, value, g = r.best("acc")
    assert (prior.tolist(), beta, value, g) == ([1.0, 0.0], 2.0, 2 / 3, 1) and r.best("f1_weighted")[3] in (1, 2)
    # float64 grids are cast once; lists of rows are taken too; the sweep and the gate sweep live side by side
    assert Evaluator(model, gate_sweep=grid.double())._gate_sweep.grid.dtype == torch.float32
    assert Evaluator(model, gate_sweep=np.array([[0.55, 0.45, 2.0]]))._gate_sweep.G == 1
    both = Evaluator(model, gate_sweep=grid, sweep=grid[:21, :2])
    assert both._sweep.G == 21 and both._gate_sweep.G == 126
    bad = {"non-negative": torch.tensor([[0.5, -0.5, 1.0]]), "finite": torch.tensor([[0.5, float("nan"), 1.0]]),
           r"\(G, 3\)": torch.zeros(4, 2), "1 <= G <= 4096": torch.zeros(4097, 3), "float32 or float64": torch.zeros(4, 3, dtype=torch.int64),
           "at most 1024": torch.tensor([[0.5, 1024.5, 1.0]]), "at most 16": torch.tensor([[0.5, 0.5, 16.5]])}
    for match, g in bad.items():
        with pytest.raises(ValueError, match=match):
            Evaluator(model, gate_sweep=g)
    for g in (torch.tensor([[0.5, 0.5, float("inf")]]), torch.tensor([[0.5, 0.5, -1.0]]), torch.zeros(0, 3), torch.zeros(3),
              torch.zeros(4, 3, dtype=torch.float16), torch.tensor([[1e39, 0.5, 1.0]], dtype=torch.float64)):
        with pytest.raises(ValueError, match="gate_sweep"):
            Evaluator(model, gate_sweep=g)
    Evaluator(model, gate_sweep=torch.tensor([[1024.0, 0.0, 16.0]]))                 # the caps themselves are inside

    class Active:                                            # a communicator with more than one rank
        active = True
    with pytest.raises(NotImplementedError, match="across ranks"):
        Evaluator(model, comm=Active(), gate_sweep=grid)

    # the apply arguments: the per-sample entropy gating only; one alone leaves the other at 1
    sample = dict(dynamic=True, dynamic_mode="sample")
    assert Evaluator(model, gate_prior=[0.55, 0.45], gate_beta=2, **sample)._gate == ([0.55, 0.45], 2.0)
    assert Evaluator(model, gate_prior=np.array([0.55, 0.45], dtype=F32), **sample)._gate == ([float(F32(0.55)), float(F32(0.45))], 1.0)
    assert Evaluator(model, gate_beta=0.5, **sample)._gate == ([1.0, 1.0], 0.5)
    assert Evaluator(model, **sample)._gate is None
    for kw in (dict(), dict(dynamic=True), dict(dynamic=True, dynamic_mode="batch"), dict(dynamic_mode="sample")):
        with pytest.raises(ValueError, match="dynamic_mode='sample'"):
            Evaluator(model, gate_prior=[0.55, 0.45], **kw)
        with pytest.raises(ValueError, match="dynamic_mode='sample'"):
            Evaluator(model, gate_beta=2.0, **kw)
    for kw, match in ((dict(gate_prior=[1.0]), "2 priors"), (dict(gate_prior=[1.0, -1.0]), "gate_prior"), (dict(gate_prior=[1.0, 2000.0]), "gate_prior"),
                      (dict(gate_prior=[float("nan"), 1.0]), "gate_prior"), (dict(gate_beta=-0.5), "gate_beta"), (dict(gate_beta=17), "gate_beta"),
                      (dict(gate_beta=float("inf")), "gate_beta")):
        with pytest.raises(ValueError, match=match):
            Evaluator(model, **kw, **sample)
