"""CPU: the fp64 restatement of SumFusion / FiLM / GatedFusion (fusion_model.py) against the reference's own modules (the fixture
golden/fusion_small.npz), the exact-input builders' conditions, and `attach_fusion` on device="cpu" models: names, shapes, order,
refusals.  No kernel runs here."""
import os

import numpy as np
import pytest
import torch

import fusion_model as F

CASES = [("sum", True), ("film", True), ("film", False), ("gated", True), ("gated", False)]


class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"
    lorb, clip, modal3 = "base", False, False


def load_case(golden_dir, method, flag):
    fx = np.load(os.path.join(golden_dir, "fusion_small.npz"))
    k = method if method == "sum" else f"{method}_{int(flag)}"
    get = lambda n: torch.from_numpy(fx[f"{k}/{n}"])                     # noqa: E731
    params = {n[len(method) + 3:]: torch.from_numpy(fx[n]) for n in fx.files if n.startswith(method + "/p/")}
    want = {n[len(k) + 1:]: torch.from_numpy(fx[n]) for n in fx.files
            if n.startswith(k + "/") and not n.startswith(k + "/p/") and n[len(k) + 1:] not in ("x", "y", "labels")}
    return get("x"), get("y"), get("labels"), params, want


@pytest.mark.parametrize("method,flag", CASES)
def test_restatement_equals_reference_fixture(method, flag, golden_dir):
    x, y, labels, params, want = load_case(golden_dir, method, flag)
    assert list(params) == list(F.param_shapes(method, 128, 6))
    got = F.run(method, x, y, params, labels, flag)
    assert set(want) >= {"out", "loss", "dlogits", "dx", "dy"} | {"d" + n for n in params}
    for n, v in want.items():
        # the hidden layers' weight gradients are stored rounded to fp32 (the fixture's size): half an fp32 ulp of their largest element
        tol = 1e-12 if v.dtype == torch.float64 else 2.0 ** -24 * v.abs().max().item()
        assert (got[n] - v.double()).abs().max().item() <= tol, n


@pytest.mark.parametrize("method,flag", CASES)
def test_exact_inputs_meet_their_conditions(method, flag):
    """check_exact_case runs inside the builder: grids, sum budgets, gate values {0, 0.5, 1}, SAT margin / UNI equality."""
    for (B, D, C) in ((1, 64, 1), (5, 320, 65), (64, 768, 128), (5, 512, 6)):
        for pattern in ("sat", "uni"):
            c = F.exact_case(method, B, D, C, pattern, flag)
            r = F.run(method, c.x, c.y, c.params, c.labels, flag, F.INV, gate=F.ExactGate.apply)
            if pattern == "sat":                                          # one-hot softmax: dlogits rounds to 0 or +-INV in fp32
                assert set(r["dlogits"].float().abs().unique().tolist()) <= {0.0, F.INV}


def _model(cls_name="AVClassifier", **over):
    import mla_hip

    class A(AVArgs):
        pass
    for k, v in over.items():
        setattr(A, k, v)
    if cls_name == "AVClassifier":
        return mla_hip.AVClassifier(A(), device="cpu", seed=0)
    if cls_name == "CLIPClassifier":
        A.clip = True
        return mla_hip.CLIPClassifier(A(), device="cpu", seed=0)
    if cls_name == "CAVClassifier":
        A.lorb = "large"
        return mla_hip.CAVClassifier(A(), device="cpu", depth=1, seed=0)
    A.dataset = "IEMOCAP" if cls_name == "Modal3Classifier" else "MVSA"
    return getattr(mla_hip, cls_name)(A(), device="cpu", depth=1, text_vocab_size=50, seed=0)


@pytest.mark.parametrize("method", ["sum", "film", "gated"])
@pytest.mark.parametrize("cls_name", ["AVClassifier", "M3AEClassifier", "CLIPClassifier", "CAVClassifier"])
def test_attach_names_shapes_order(method, cls_name):
    import mla_hip
    model = _model(cls_name)
    before = [k for k in model.state_dict() if not k.startswith("fusion_module.")]
    D, C = model.feat_dim, model.fusion_module.fc_out.out_features
    fusion = mla_hip.attach_fusion(model, method, seed=3)
    assert model.fusion_module is fusion and fusion.method == method
    sd = model.state_dict()
    shapes = F.param_shapes(method, D, C)
    fkeys = [k for k in sd if k.startswith("fusion_module.")]
    assert fkeys == ["fusion_module." + k for k in shapes]                                  # the reference's names and order
    assert [k for k in sd if not k.startswith("fusion_module.")] == before                  # nothing else moved
    assert list(sd)[:len(fkeys)] == fkeys                                                   # where the reference's fusion_module sits
    for k, shp in shapes.items():
        assert tuple(sd["fusion_module." + k].shape) == shp
    named = dict(model.named_parameters())
    assert [k for k in named if k.startswith("fusion_module.")] == fkeys
    # one flat owner, every parameter a view of it, in order; xavier-normal weights, zero biases, seeded
    off = 0
    for k in shapes:
        p = named["fusion_module." + k]
        assert isinstance(p, torch.nn.Parameter) and p._mla_owner is fusion
        assert p.untyped_storage().data_ptr() == fusion.flat.untyped_storage().data_ptr() and p.storage_offset() == off
        off += p.numel()
        if k.endswith("bias"):
            assert not p.detach().any()
        else:
            std = (2.0 / sum(p.shape)) ** 0.5
            assert 0.8 * std < p.detach().std().item() < 1.2 * std
    assert off == fusion.numel
    again = mla_hip.attach_fusion(_model(cls_name), method, seed=3)
    assert torch.equal(again.flat, fusion.flat)
    assert isinstance(fusion.fc_out if method != "sum" else fusion.fc_x, torch.nn.Linear)
    model.load_state_dict(sd)
    opt = mla_hip.FusedSGD(model.parameters(), lr=1e-3)                                     # the head is ONE optimiser group
    assert sum(1 for g in opt.groups.values() if g is fusion) == 1


def test_attach_refusals():
    import mla_hip
    from mla_hip import MLAHipError
    with pytest.raises(MLAHipError, match="gs_flag false"):
        mla_hip.attach_fusion(_model(gs_flag=True), "sum")
    with pytest.raises(MLAHipError, match="two inputs"):
        mla_hip.attach_fusion(_model("Modal3Classifier"), "film")
    m = _model()
    mla_hip.attach_qmf_heads(m, seed=1)
    with pytest.raises(MLAHipError, match="QMF heads"):
        mla_hip.attach_fusion(m, "gated")
    m = _model()
    mla_hip.attach_fusion(m, "sum")
    with pytest.raises(MLAHipError, match="already has an attached sum fusion"):
        mla_hip.attach_fusion(m, "film")
    with pytest.raises(MLAHipError, match="attached sum / film / gated fusion"):
        mla_hip.attach_qmf_heads(m)
    with pytest.raises(MLAHipError, match="method must be one of"):
        mla_hip.attach_fusion(_model(), "concat")


@pytest.mark.parametrize("method", ["film", "gated"])
def test_trainers_refuse_what_the_reference_does_not_define(method):
    import mla_hip
    m = _model("CLIPClassifier")
    mla_hip.attach_fusion(m, method)
    for mod in ("OGM", "OGM_GE"):
        with pytest.raises(NotImplementedError, match="no per-modality"):
            mla_hip.JointTrainer(m, modulation=mod)

    comm = mla_hip.Comm()
    comm.world = 2
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mla_hip.JointTrainer(m, comm=comm)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mla_hip.JointEvaluator(m, comm=comm)


@pytest.mark.parametrize("fusion", ["sum", "film", "gated"])
def test_constructors_still_raise(fusion):
    import mla_hip
    for name in ("AVClassifier", "CLIPClassifier", "M3AEClassifier"):
        with pytest.raises(NotImplementedError, match="Incorrect fusion method: {}!".format(fusion)):
            _model(name, fusion_method=fusion)
    assert {"fusion_sum_ce_fwd_bwd", "fusion_film_fwd", "fusion_gated_bwd"} <= set(mla_hip.torch_ops.op_names())
