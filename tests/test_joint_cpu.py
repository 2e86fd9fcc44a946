"""CPU: the joint concat-fusion (gs_flag false) model objects -- construction, reference state_dict layout, what stays
unsupported -- and the self-consistency of the joint fixture (tests/golden/joint_small.npz, make_golden_joint.py)."""
import os

import numpy as np
import pytest
import torch


class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"


class M3AEArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "Food101", False, "Normal"


class Modal3Args:
    fusion_method, dataset, gs_flag, modulation = "concat", "IEMOCAP", False, "Normal"


def test_classifiers_construct_without_gs_flag():
    from mla_hip import AVClassifier, M3AEClassifier, Modal3Classifier
    from mla_hip.m3ae import ConcatFusion3
    from mla_hip.model import ConcatFusion
    av = AVClassifier(AVArgs(), device="cpu", seed=0)
    assert isinstance(av.fusion_module, ConcatFusion) and av.fusion_module.joint
    assert av.fusion_module.fc_out.weight.shape == (6, 1024)                     # basic_model.py:33-34
    m3 = M3AEClassifier(M3AEArgs(), device="cpu", depth=1, text_vocab_size=64, seed=0)
    assert m3.fusion_module.fc_out.weight.shape == (101, 1536)                   # basic_model.py:152-154
    m3d = Modal3Classifier(Modal3Args(), device="cpu", depth=1, text_vocab_size=64, seed=0)
    assert isinstance(m3d.fusion_module, ConcatFusion3) and m3d.fusion_module.joint
    assert m3d.fusion_module.fc_out.weight.shape == (4, 2304)                    # basic_model.py:221-223
    for modulation in ("OGM", "OGM_GE"):
        class A(AVArgs):
            pass
        A.modulation = modulation
        assert AVClassifier(A(), device="cpu", seed=0).fusion_module.fc_out.weight.shape == (6, 1024)


def test_gs_flag_objects_unchanged():
    from mla_hip import AVClassifier

    class A(AVArgs):
        gs_flag = True
    m = AVClassifier(A(), device="cpu", seed=0)
    assert m.fusion_module.fc_out.weight.shape == (6, 512) and not m.fusion_module.joint
    with pytest.raises(NotImplementedError, match="gs_flag"):
        m.fusion_module(torch.zeros(2, 512), torch.zeros(2, 512))


def test_out_of_scope_configurations_raise():
    from mla_hip import AVClassifier, M3AEClassifier

    class QMF(AVArgs):
        modulation = "QMF"
    with pytest.raises(NotImplementedError, match="QMF"):
        AVClassifier(QMF(), device="cpu")

    class M3QMF(M3AEArgs):
        modulation = "QMF"
    with pytest.raises(NotImplementedError, match="QMF"):
        M3AEClassifier(M3QMF(), device="cpu", depth=1, text_vocab_size=64)

    class Sum(AVArgs):
        fusion_method = "sum"
    with pytest.raises(NotImplementedError, match="Incorrect fusion method"):
        AVClassifier(Sum(), device="cpu")

    class Large(AVArgs):
        lorb = "large"
    with pytest.raises(NotImplementedError, match="large"):
        AVClassifier(Large(), device="cpu")

    class Clip(AVArgs):
        clip = True
    with pytest.raises(NotImplementedError, match="clip"):
        AVClassifier(Clip(), device="cpu")

    from mla_hip import JointTrainer
    with pytest.raises(NotImplementedError, match="QMF"):
        JointTrainer(AVClassifier(AVArgs(), device="cpu", seed=0), modulation="QMF")


def test_joint_trainer_rejects_gs_flag_models():
    from mla_hip import AVClassifier, JointTrainer
    from mla_hip._lib import MLAHipError

    class A(AVArgs):
        gs_flag = True
    with pytest.raises(MLAHipError, match="gs_flag"):
        JointTrainer(AVClassifier(A(), device="cpu", seed=0))


def test_state_dict_matches_the_reference_and_roundtrips(golden_dir):
    from mla_hip import AVClassifier
    fx = np.load(os.path.join(golden_dir, "joint_small.npz"))
    keys = [str(k) for k in fx["state_keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",") if d) for s in fx["state_shapes"]]
    m = AVClassifier(AVArgs(), device="cpu", seed=0)
    sd = m.state_dict(prefix="module.")                               # torch.nn.DataParallel's keys (main.py:921)
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sd["module.fusion_module.fc_out.weight"].shape == (6, 1024)
    m2 = AVClassifier(AVArgs(), device="cpu", seed=1)
    assert not torch.equal(m2.fusion_module.fc_out.weight, m.fusion_module.fc_out.weight)
    m2.load_state_dict(sd)                                            # `module.` prefix accepted (main.py:724)
    sd2 = m2.state_dict()
    for k, v in sd.items():
        assert torch.equal(sd2[k[len("module."):]], v), k


def test_joint_fixture_is_self_consistent(golden_dir):
    from oracle import mla_oracle as O
    fx = np.load(os.path.join(golden_dir, "joint_small.npz"))
    cases = [(tag, [int(x) for x in fx[f"{tag}.meta"]]) for tag in ("normal", "ogm", "m3ae")]
    for tag, meta in cases:
        if tag == "m3ae":
            B, _depth, _vocab, C, steps, seed = meta
            lab_of = lambda s: O.portable_labels(seed + 50 + s, B, C).numpy()              # noqa: E731
            D = 768
        else:
            B, *_rest, steps, seed = meta
            C, D = 6, 512
            lab_of = lambda s: O.portable_labels(seed + 100 + s, B, 6).numpy()             # noqa: E731
        for s in range(steps):
            p = f"{tag}.s{s}."
            out, oa, ov = fx[p + "out"].astype(np.float64), fx[p + "out_a"], fx[p + "out_v"]
            assert out.shape == (B, C) and fx[p + "a"].shape == (B, D)
            np.testing.assert_allclose(out, oa.astype(np.float64) + ov, atol=1e-5)
            # the recorded gradients restated from a, v, out and the labels: dlogits = (softmax(out) - onehot) / B,
            # dW = dlogits^T cat(a, v) (column block m multiplies modality m), db = sum dlogits, loss = mean CE
            lab = lab_of(s)
            e = np.exp(out - out.max(axis=1, keepdims=True))
            sm = e / e.sum(axis=1, keepdims=True)
            dl = (sm - np.eye(C)[lab]) / B
            cat = np.concatenate([fx[p + "a"], fx[p + "v"]], axis=1).astype(np.float64)
            np.testing.assert_allclose(fx[p + "head_grad"], dl.T @ cat, atol=1e-6)
            np.testing.assert_allclose(fx[p + "head_bias_grad"], dl.sum(axis=0), atol=1e-7)
            np.testing.assert_allclose(float(fx[p + "loss"]), -np.log(sm[np.arange(B), lab]).mean(), atol=1e-6)
        if tag == "ogm":
            for s in range(steps):
                c = fx[f"ogm.s{s}.coeff"]
                assert sorted(c.tolist())[1] == 1.0 and 0.0 < min(c) < 1.0                     # one modality damped
    # OGM rescales conv gradients only after the forward / backward: step 0 features and losses agree across the cases
    np.testing.assert_array_equal(fx["normal.s0.out"], fx["ogm.s0.out"])
