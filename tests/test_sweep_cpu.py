"""CPU: the closed forms of the fusion-sweep restatement (tests/sweep_model.py), fusion_grid, SweepResult, the refusals of the additive
ABI entry mla_fusion_sweep (nothing is dereferenced before validation), `make host-check`, and Evaluator's sweep= argument rules."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import sweep_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_one_grid_row_reproduces_a_modality_and_ties_go_to_the_lower_class():
    rng = np.random.default_rng(0)
    M, B, C = 3, 40, 5
    outs = rng.standard_normal((M, B, C)).astype(F32)
    labels = rng.integers(0, C, size=B)
    grid = np.eye(M, dtype=F32)
    for fused in (False, True):
        tp, pp, num = SM.sweep(outs, labels, grid, fused=fused)
        assert (num == np.bincount(labels, minlength=C)).all()
        for m in range(M):
            arg = outs[m].argmax(axis=1)
            assert (pp[m] == np.bincount(arg, minlength=C)).all()
            assert (tp[m] == np.bincount(labels[arg == labels], minlength=C)).all()
    # duplicates: the lower index, also when the fused values are all +0.0 (the zero grid row) or all equal
    tied = np.zeros((2, 3, 4), dtype=F32)
    tied[:, 0] = [1, 7, 7, 3]
    tied[:, 1] = [5, 5, 5, 5]
    tied[:, 2] = [-2, -9, -2, -2]
    pred = SM.predict(tied, np.array([0, 0, 0]), np.array([[0.5, 0.5], [0, 0], [1, 0]], dtype=F32))
    assert pred.tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert SM.first_max(np.array([[-np.inf, -np.inf]])).tolist() == [0]


def test_bad_labels_empty_rows_and_zero_eligible_sums_follow_the_policies():
    M, C = 3, 4
    outs = np.zeros((M, 6, C), dtype=F32)
    outs[0, :, 1] = 1                                        # modality 0 says class 1, modality 1 class 2, modality 2 class 3
    outs[1, :, 2] = 1
    outs[2, :, 3] = 1
    labels = np.array([1, -1, C, 2 ** 40, 2, 3], dtype=np.int64)
    present = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 1, 0]], dtype=np.uint8)
    grid = np.array([[1, 0, 0], [0, 1, 0], [0.25, 0.25, 0.5]], dtype=F32)
    assert SM.row_counted(labels, C, present).tolist() == [True, False, False, False, False, True]
    pred = SM.predict(outs, labels, grid, present)
    # rows 1-4 are counted nowhere; row 5 has only modality 1: grid row 0 gives it no share (left out), rows 1 and 2 renormalise to it
    assert pred.tolist() == [[1, -1, -1, -1, -1, -1], [2, -1, -1, -1, -1, 2], [3, -1, -1, -1, -1, 2]]
    tp, pp, num = SM.count_tables(pred, labels, C, present)
    assert num.tolist() == [0, 1, 0, 1]                      # row 5 stays in num for every grid row
    assert pp.tolist() == [[0, 1, 0, 0], [0, 0, 2, 0], [0, 0, 1, 1]] and tp.tolist() == [[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    w, ok = SM.pair_weights(grid, 6, present)
    assert ok[:, 5].tolist() == [False, True, True] and w[2, 5].tolist() == [0.0, 1.0, 0.0] and w[2, 0].tolist() == [0.25, 0.25, 0.5]
    # without a present matrix every modality takes part and only the labels decide
    assert SM.row_counted(labels, C).tolist() == [True, False, False, False, True, True]


def test_the_two_roundings_differ_exactly_where_the_near_tie_is_built():
    """Grid row (1, 1 + 2^-12); class A = (-1, 1 + 2^-12), class B = (2^-11 + 2^-25, 0).  Unfused A = 2^-11 < B, fused
    A = 2^-11 + 2^-24 > B."""
    e = F32(2.0 ** -12)
    grid = np.array([[1, F32(1) + e]], dtype=F32)
    outs = np.zeros((2, 1, 2), dtype=F32)
    outs[:, 0, 0] = [-1, F32(1) + e]
    outs[:, 0, 1] = [F32(2.0 ** -11 + 2.0 ** -25), 0]
    w, _ = SM.pair_weights(grid, 1)
    assert SM.fuse(w, outs)[0, 0].tolist() == [2.0 ** -11, 2.0 ** -11 + 2.0 ** -25]
    assert SM.fuse(w, outs, fused=True)[0, 0].tolist() == [2.0 ** -11 + 2.0 ** -24, 2.0 ** -11 + 2.0 ** -25]
    assert SM.predict(outs, [0], grid).tolist() == [[1]] and SM.predict(outs, [0], grid, fused=True).tolist() == [[0]]
    # exactly-summable inputs: the two forms agree
    o, lab, g = SM.exact_case(3, 9, 7, 12, seed=1)
    assert (SM.predict(o, lab, g) == SM.predict(o, lab, g, fused=True)).all()
    assert np.abs(o).max() <= 512 and (o == np.round(o)).all() and (g * 256 == np.round(g * 256)).all() and g.min() >= 0 and g.max() <= 1


# ---- fusion_grid ---------------------------------------------------------------------------------------------------------------------
def test_fusion_grid_rows_and_the_two_modality_identity():
    from mla_hip import fusion_grid
    for steps in (10, 20, 50, 100):
        g = fusion_grid(2, steps)
        assert g.dtype == torch.float32 and tuple(g.shape) == (steps + 1, 2) and not g.is_cuda
        for k in range(steps + 1):
            a = k / steps
            want = np.array([a, 1.0 - a]).astype(F32)        # what Evaluator(av_alpha=a) hands the kernels: [a, 1.0 - a] as C floats
            assert g[k].numpy().tobytes() == want.tobytes(), (steps, k)
    for steps in (1, 4, 20, 80):
        g = fusion_grid(3, steps).numpy()
        assert g.shape == ((steps + 1) * (steps + 2) // 2, 3) and g.dtype == F32
        rows = [(i, j) for i in range(steps + 1) for j in range(steps + 1 - i)]             # i outer, j inner
        want = np.array([(i / steps, j / steps, (steps - i - j) / steps) for i, j in rows]).astype(F32)
        assert g.tobytes() == want.tobytes()
        assert np.abs(g.astype(F64).sum(axis=1) - 1).max() <= 2.0 ** -23                    # within one ulp of 1
        assert g.min() >= 0
    assert fusion_grid(3, 80).shape[0] == 3321 and fusion_grid(3, 20).shape[0] == 231
    with pytest.raises(ValueError, match="2 or 3"):
        fusion_grid(4, 10)
    with pytest.raises(ValueError, match="steps"):
        fusion_grid(2, 0)


# ---- SweepResult ---------------------------------------------------------------------------------------------------------------------
def test_sweep_result_f1_is_f1_from_confusion_and_best_is_the_first_maximum():
    from mla_hip import SweepResult
    from mla_hip.metrics import f1_from_confusion
    rng = np.random.default_rng(5)
    M, B, C, G = 2, 300, 5, 9
    outs = rng.standard_normal((M, B, C)).astype(F32)
    outs[:, :, 4] = -50                                      # class 4 is never predicted ...
    labels = rng.integers(0, C - 2, size=B)                  # ... and classes 3, 4 never a label: 3 is predicted only
    present = (rng.random((B, M)) < 0.7).astype(np.uint8)
    grid = np.stack([np.linspace(0, 1, G), 1 - np.linspace(0, 1, G)], axis=1).astype(F32)
    grid[5] = grid[4]                                        # a tie between two grid rows
    pred = SM.predict(outs, labels, grid)
    tp, pp, num = SM.count_tables(pred, labels, C)
    s = SweepResult(grid, tp, pp, num)
    assert s.acc.dtype == F64 and s.acc.shape == (G,) and s.counted.dtype == np.int64
    assert (s.acc == tp.sum(axis=1) / num.sum()).all() and (s.counted == B).all()
    for average in ("macro", "weighted"):
        f = s.f1(average)
        assert f.dtype == F64 and f.shape == (G,)
        for g in range(G):
            conf = SM.confusion_of(pred[g], labels, C)
            assert (conf.sum(axis=1) == num).all() and (conf.sum(axis=0) == pp[g]).all() and (np.diag(conf) == tp[g]).all()
            assert f[g] == f1_from_confusion(conf[None], average)[0]
    # pairs that were left out count as errors: the row stays in num (the denominators) and in no pp
    predp = SM.predict(outs, labels, grid, present)
    left = SweepResult(grid, *SM.count_tables(predp, labels, C, present))
    assert (left.counted[[0, G - 1]] < left.num.sum()).all() and (left.counted[1:G - 1] == left.num.sum()).all()   # (0, 1) and (1, 0)
    assert (left.acc == left.tp.sum(axis=1) / left.num.sum()).all() and (left.acc[[0, G - 1]] <= left.counted[[0, G - 1]] / left.num.sum()).all()
    tiny = SweepResult(grid[:1], np.array([[1, 0]]), np.array([[1, 0]]), np.array([2, 2]))        # 4 rows, 1 predicted (right), 3 left out
    assert tiny.acc.tolist() == [0.25] and tiny.counted.tolist() == [1]
    assert tiny.f1("macro").tolist() == [(2 / 3 + 0) / 2] and tiny.f1("weighted").tolist() == [(2 / 3 * 2 + 0 * 2) / 4]
    with pytest.raises(ValueError, match="macro"):
        s.f1("micro")
    for metric, v in (("acc", s.acc), ("f1_macro", s.f1("macro")), ("f1_weighted", s.f1("weighted"))):
        w, value, g = s.best(metric)
        assert value == v.max() and g == int(np.flatnonzero(v == v.max())[0]) and (w == grid[g]).all()
    tie = SweepResult(grid[:3], np.array([[1, 0], [2, 0], [2, 0]]), np.array([[2, 1], [3, 0], [3, 0]]), np.array([2, 1]))
    assert tie.best("acc")[1:] == (2 / 3, 1) and tie.best("f1_macro")[2] == 1 and tie.best("f1_weighted")[2] == 1
    with pytest.raises(ValueError, match="metric"):
        s.best("map")
    empty = SweepResult(grid[:2], np.zeros((2, 3), np.int64), np.zeros((2, 3), np.int64), np.zeros(3, np.int64))
    assert empty.acc.tolist() == [0.0, 0.0] and empty.f1().tolist() == [0.0, 0.0] and empty.best()[1:] == (0.0, 0)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_abi_entry_is_additive_and_refuses_before_any_launch():
    from mla_hip import _lib, torch_ops
    lib = _lib.load()
    assert hasattr(lib, "mla_fusion_sweep") and len(_lib.PROTOTYPES["mla_fusion_sweep"][1]) == 14
    assert lib.mla_abi_version() == 3                        # additive
    assert "fusion_sweep" in torch_ops.op_names()
    fake = 0x1000                                            # non-null, aligned, never dereferenced: validation fails first
    err = lib.mla_last_error

    def sweep(l0=fake, l1=fake, l2=fake, labels=fake, present=None, grid=fake, tp=fake, pp=fake, num=None, M=3, B=4, C=6, G=8):
        return lib.mla_fusion_sweep(l0, l1, l2, labels, present, grid, tp, pp, num, M, B, C, G, None)
    for M in (0, 1, 4, -2):
        assert sweep(M=M) == -1 and f"mla_fusion_sweep: need M = 2 or 3 (got {M})".encode() in err()
    for null in ("l0", "l1", "l2", "labels", "grid", "tp", "pp"):
        assert sweep(**{null: None}) == -1 and b"mla_fusion_sweep: null pointer" in err(), null
    for null in ("l0", "l1", "labels", "grid", "tp", "pp"):
        assert sweep(M=2, l2=None, **{null: None}) == -1 and b"mla_fusion_sweep: null pointer" in err(), null
    for name in ("B", "C", "G"):
        for v in (0, -1):
            assert sweep(**{name: v}) == -1 and b"mla_fusion_sweep: need" in err(), (name, v)
    assert sweep(C=129) == -1 and b"mla_fusion_sweep: need 0 < C <= 128 (got 129)" in err()
    assert sweep(G=4097) == -1 and b"mla_fusion_sweep: need 0 < G <= 4096 grid points (got 4097)" in err()
    for off in ("l0", "l1", "l2", "grid", "tp", "pp"):
        assert sweep(**{off: fake + 2}) == -1 and b"4-byte" in err(), off
    assert sweep(num=fake + 2) == -1 and b"4-byte" in err()
    assert sweep(labels=fake + 4) == -1 and b"8-byte" in err()
    with pytest.raises(Exception):                           # no CPU implementation: torch's "no kernel" error
        torch.ops.mla_hip.fusion_sweep(torch.zeros(2, 4, 3), torch.zeros(4, dtype=torch.int64), torch.zeros(5, 2),
                                       torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int32))


def test_host_check_builds_and_runs_the_sweep_program():
    csrc = os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "host-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep host check ok" in r.stdout and "sweep_host_check.cpp" in r.stdout and "-fsanitize=address,undefined" in r.stdout


# ---- Evaluator's argument rules ------------------------------------------------------------------------------------------------------
class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "CREMAD", True, "Normal", True


def test_evaluator_takes_sweep_and_defaults_to_nothing():
    from mla_hip import CLIPClassifier, Evaluator, FusionSweep, SweepResult, fusion_grid
    from mla_hip._lib import MLAHipError
    assert inspect.signature(Evaluator.__init__).parameters["sweep"].default is None
    model = CLIPClassifier(ClipArgs(), device="cpu", seed=0, feat_dim=64)
    ev = Evaluator(model)
    assert ev._sweep is None
    with pytest.raises(MLAHipError, match="sweep=None"):
        ev.sweep_result()
    ev.reset()                                               # nothing to zero
    grid = fusion_grid(2, 20)
    ev = Evaluator(model, av_alpha=0.55, sweep=grid)         # host tensors: nothing is launched before the first update
    sw = ev._sweep
    assert isinstance(sw, FusionSweep) and (sw.M, sw.C, sw.G) == (2, 6, 21)
    assert sw.tp.shape == (21, 6) and sw.pp.shape == (21, 6) and sw.num.shape == (6,)
    assert sw.tp.dtype == sw.pp.dtype == sw.num.dtype == torch.int32 and torch.equal(sw.grid, grid)
    s = ev.sweep_result()                                    # empty tables answer zeros
    assert isinstance(s, SweepResult) and s.weights.dtype == F32 and s.weights.shape == (21, 2)
    assert s.tp.dtype == s.pp.dtype == s.num.dtype == s.counted.dtype == np.int64
    assert s.tp.shape == (21, 6) and s.num.shape == (6,) and s.acc.tolist() == [0.0] * 21 and s.best("acc")[2] == 0
    sw.tp += 1
    ev.reset()
    assert int(sw.tp.sum()) == 0
    # float64 grids are cast once; lists of rows are taken too
    assert Evaluator(model, sweep=grid.double())._sweep.grid.dtype == torch.float32
    assert Evaluator(model, sweep=np.array([[0.55, 0.45]]))._sweep.G == 1
    bad = {"non-negative": torch.tensor([[0.5, -0.5]]), "finite": torch.tensor([[0.5, float("nan")]]),
           r"\(G, 2\)": torch.zeros(4, 3), "1 <= G <= 4096": torch.zeros(4097, 2), "float32 or float64": torch.zeros(4, 2, dtype=torch.int64)}
    for match, g in bad.items():
        with pytest.raises(ValueError, match=match):
            Evaluator(model, sweep=g)
    for g in (torch.tensor([[0.5, float("inf")]]), torch.zeros(0, 2), torch.zeros(2), torch.zeros(4, 2, dtype=torch.float16)):
        with pytest.raises(ValueError, match="sweep"):
            Evaluator(model, sweep=g)

    class Active:                                            # a communicator with more than one rank
        active = True
    with pytest.raises(NotImplementedError, match="across ranks"):
        Evaluator(model, comm=Active(), sweep=grid)
    Evaluator(model, comm=Active())                          # without a sweep an active comm is what it was
