"""CPU: the `--clip` model (CLIPClassifier on stored features) -- the reference fixture against the restatement in
tests/clip_model.py, the additive ABI entries, the model's keys / shapes / refusals and the batcher's host half."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import mla_oracle as O
from util import assert_close
import clip_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ClipArgs:
    fusion_method, dataset, gs_flag, modulation, clip = "concat", "Food101", True, "Normal", True


@pytest.mark.parametrize("tag,gs_mode", [("intended", "as_intended"), ("published", "as_published")])
def test_fixture_equals_restatement(tag, gs_mode, golden_dir):
    """clip_small.npz holds what the reference's own CLIPClassifier / GSPlugin / torch.optim.SGD computed over main.py:428-454; the
    restatement must reproduce it to the tolerances its maker asserted (CPU vs CPU: 2e-6 + 2e-4 rel on logits and losses, Pl 1e-8 +
    1e-4 rel, head and momentum 1e-7 + 1e-6 rel)."""
    fx = np.load(os.path.join(golden_dir, "clip_small.npz"))
    B, D, C, steps, seed, ldl = [int(v) for v in fx["meta"]]
    st = R.ClipState(O.make_head_params(D, C, seed + 2), D)
    for s in range(steps):
        tok, img, label = R.clip_inputs(seed, s, B, D, C)
        rec = R.clip_gs_step(st, tok, img, label, s, ldl, gs_mode=gs_mode)
        for k in ("out_a", "out_v", "loss_a", "loss_v", "loss"):
            assert_close(rec[k], fx[f"{tag}.s{s}.{k}"], atol=2e-6, rtol=2e-4, name=f"{tag} s{s} {k}")
        assert_close(st.Pl[:8, :8], fx[f"{tag}.s{s}.Pl.corner"], atol=1e-8, rtol=1e-4, name="Pl corner")
        assert_close(st.Pl[::16, ::16], fx[f"{tag}.s{s}.Pl.sub"], atol=1e-8, rtol=1e-4, name="Pl sub")
        assert abs(torch.linalg.norm(st.Pl).item() - float(fx[f"{tag}.s{s}.Pl.fro"])) < 1e-5
    if gs_mode == "as_published":
        assert torch.equal(st.Pl, torch.eye(D))
        pick, sfx = (lambda t: t[:, ::4]), ".col4"
        assert abs(st.head["weight"].double().abs().sum().item() - float(fx[f"{tag}.head.weight.abssum"])) < 1e-3
        assert abs(st.mom["weight"].double().abs().sum().item() - float(fx[f"{tag}.momentum.weight.abssum"])) < 1e-3
    else:
        pick, sfx = (lambda t: t), ""
    assert_close(pick(st.head["weight"]), fx[f"{tag}.head.weight{sfx}"], atol=1e-7, rtol=1e-6, name="head weight")
    assert_close(pick(st.mom["weight"]), fx[f"{tag}.momentum.weight{sfx}"], atol=1e-7, rtol=1e-6, name="weight momentum")
    assert_close(st.head["bias"], fx[f"{tag}.head.bias"], atol=1e-7, rtol=1e-6, name="head bias")
    assert_close(st.mom["bias"], fx[f"{tag}.momentum.bias"], atol=1e-7, rtol=1e-6, name="bias momentum")


def test_fixture_is_small_data(golden_dir):
    path = os.path.join(golden_dir, "clip_small.npz")
    assert os.path.getsize(path) <= 700 * 1024
    fx = np.load(path, allow_pickle=False)                   # data only: plain numeric arrays
    assert all(fx[k].dtype.kind in "fi" for k in fx.files)


def test_abi_exports_the_feature_entries():
    import ctypes
    from mla_hip import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "mla_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {"mla_feature_ws_elems": 3, "mla_feature_phase": 20, "mla_gather_index_check": 3, "mla_gather_rows2": 12}
    for name, arity in want.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, f"{name} is not declared in include/mla_hip.h"
        assert len(m.group(1).split(",")) == arity == len(_lib.PROTOTYPES[name][1]), name
    assert lib.mla_abi_version() == 3                        # additive
    # host-side sizing and validation answer without a GPU
    assert lib.mla_feature_ws_elems(64, 512, 101) == 64 * 101 + 64 + 6 * 512 + 101 * 512       # three fp64 vectors of D
    assert lib.mla_feature_ws_elems(5, 70, 65) == 332 + 6 * 70 + 65 * 70                             # 5 * 65 + 5 = 330, padded to 16 bytes
    fake = 0x1000                                            # non-null, 16-byte aligned, never dereferenced: validation fails first
    call = lambda C, w=fake: lib.mla_feature_phase(fake, fake, w, fake, fake, fake, fake, fake, fake, 4, 512, C, 0.25, 1, 0.1, 1e-3, 0.9,
                                                   1e-4, 1, None)      # noqa: E731
    assert call(129) == -1 and b"need 0 < C <= 128 (got 129)" in lib.mla_last_error()
    assert call(0) == -1
    assert call(101, fake + 4) == -1 and b"16-byte aligned" in lib.mla_last_error()
    assert lib.mla_feature_phase(None, fake, fake, fake, fake, fake, fake, fake, fake, 4, 512, 101, 0.25, 1, 0.1, 1e-3, 0.9, 1e-4, 1,
                                 None) == -1 and b"null pointer" in lib.mla_last_error()
    idx = (ctypes.c_int64 * 4)(0, 3, 1, 4)
    assert lib.mla_gather_index_check(idx, 4, 5) == 0
    assert lib.mla_gather_index_check(idx, 4, 4) == -1 and b"index 4 at position 3" in lib.mla_last_error()
    from mla_hip import torch_ops
    assert {"feature_phase", "gather_rows2"} <= set(torch_ops.op_names())


def test_clip_classifier_keys_shapes_and_refusals():
    from mla_hip import AVClassifier, CLIPClassifier, JointTrainer, MLATrainer
    from mla_hip._lib import MLAHipError
    for dataset, C in (("Food101", 101), ("MVSA", 3), ("CREMAD", 6)):
        for gs_flag, width in ((True, 512), (False, 1024)):
            A = type("A", (ClipArgs,), dict(dataset=dataset, gs_flag=gs_flag))
            m = CLIPClassifier(A(), device="cpu", seed=0)
            sd = {k: v.clone() for k, v in m.state_dict().items()}           # state_dict() hands out views of the flat buffer
            assert list(sd.keys()) == ["fusion_module.fc_out.weight", "fusion_module.fc_out.bias"]      # the reference's two keys
            assert sd["fusion_module.fc_out.weight"].shape == (C, width) and sd["fusion_module.fc_out.bias"].shape == (C,)
            assert [n for n, _p in m.named_parameters()] == list(sd.keys())
            m.load_state_dict({"module." + k: v + 1 for k, v in sd.items()})                              # main.py:724
            assert torch.equal(m.state_dict()["fusion_module.fc_out.bias"], sd["fusion_module.fc_out.bias"] + 1)
    assert CLIPClassifier(type("A", (), dict(fusion_method="concat", gs_flag=True))(), device="cpu").fusion_module.fc_out.out_features == 101
    m = CLIPClassifier(ClipArgs(), device="cpu", seed=0, feat_dim=768)                                    # ViT-L features
    assert m.fusion_module.fc_out.weight.shape == (101, 768) and m.feature_only
    assert [(t, e) for t, _g, e in m.mla_encoders()] == [("a", None), ("v", None)]
    # forward: squeeze dim 1 (basic_model.py:313-319), the tensors themselves under gs_flag
    tok, img, _ = R.clip_inputs(3, 0, 4, 768, 101)
    a, v = m(tok, img)
    ra, rv = R.clip_forward(tok, img, True)
    assert torch.equal(a, ra) and torch.equal(v, rv) and a.shape == (4, 768)
    for bad in (tok.half(), tok.double(), tok.expand(4, 2, 768), tok[..., :512], tok.reshape(4, 768, 1)):
        with pytest.raises(MLAHipError, match="float32"):
            m(bad, img)
    with pytest.raises(MLAHipError, match="batch mismatch"):
        m(tok, img[:2])
    # what is refused, and how
    for dataset in ("KineticSound", "CUB", "Food-101"):
        with pytest.raises(NotImplementedError, match="Incorrect dataset name"):
            CLIPClassifier(type("A", (ClipArgs,), dict(dataset=dataset))(), device="cpu")
    for fusion in ("sum", "film", "gated"):
        with pytest.raises(NotImplementedError, match="Incorrect fusion method"):
            CLIPClassifier(type("A", (ClipArgs,), dict(fusion_method=fusion))(), device="cpu")
    for gs_flag in (True, False):
        with pytest.raises(NotImplementedError, match="QMF"):
            CLIPClassifier(type("A", (ClipArgs,), dict(modulation="QMF", gs_flag=gs_flag))(), device="cpu")
    AV = type("AV", (), dict(fusion_method="concat", dataset="CREMAD", gs_flag=False, modulation="Normal", clip=True))
    with pytest.raises(NotImplementedError, match="clip"):
        AVClassifier(AV(), device="cpu")
    # trainers: a feature-only model has a head group and nothing else; data parallel is refused
    tr = MLATrainer(CLIPClassifier(ClipArgs(), device="cpu", seed=0))
    assert list(tr.optimizer.groups) == ["head"] and tr.fused_feature_phase and not tr._estreams
    with pytest.raises(NotImplementedError, match="data-parallel"):
        MLATrainer(CLIPClassifier(ClipArgs(), device="cpu", seed=0), comm=type("C", (), dict(world=2, active=True))())
    J = type("J", (ClipArgs,), dict(gs_flag=False, modulation="OGM_GE"))
    assert JointTrainer(CLIPClassifier(J(), device="cpu", seed=0), modulation="OGM_GE").M == 2


def test_fused_switch_is_read_at_construction(monkeypatch):
    from mla_hip import CLIPClassifier, MLATrainer
    monkeypatch.setenv("MLA_FEATURE_FUSED", "0")
    tr = MLATrainer(CLIPClassifier(ClipArgs(), device="cpu", seed=0))
    assert not tr.fused_feature_phase and not tr._fused_ok()
    monkeypatch.delenv("MLA_FEATURE_FUSED")
    assert not tr.fused_feature_phase                        # construction time, not call time
    tr = MLATrainer(CLIPClassifier(ClipArgs(), device="cpu", seed=0))
    assert tr._fused_ok()
    tr.keep_debug = True
    assert not tr._fused_ok()
    assert not MLATrainer(CLIPClassifier(ClipArgs(), device="cpu", seed=0), optimizer="adam")._fused_ok()


def _write(root, name, arr):
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, name + ".npy"), arr)


def test_batcher_host_half(tmp_path):
    from mla_hip import CLIPFeatureBatcher, epoch_permutation, load_feature_tables
    from mla_hip._lib import MLAHipError
    text, vis = str(tmp_path / "text"), str(tmp_path / "visual")
    names = [f"s{i:02d}" for i in range(11)]
    rng = np.random.default_rng(0)
    for i, n in enumerate(names):                            # (1, D) and (D,), fp32 and fp16
        t = rng.standard_normal((1, 70)).astype(np.float32)
        _write(text, n, t if i % 2 else t.reshape(70))
        _write(vis, n, rng.standard_normal((1, 70)).astype(np.float16 if i % 3 == 0 else np.float32))
    tok, img = load_feature_tables(names, text, vis)
    assert tok.shape == img.shape == (11, 70) and tok.dtype == img.dtype == torch.float32
    for i, n in enumerate(names):
        assert np.array_equal(tok[i].numpy(), np.load(os.path.join(text, n + ".npy")).reshape(70))
        assert np.array_equal(img[i].numpy(), np.load(os.path.join(vis, n + ".npy")).reshape(70).astype(np.float32))   # fp16 widened exactly
    for what, arr in (("shape", np.zeros((2, 70), np.float32)), ("shape3", np.zeros((1, 1, 70), np.float32)),
                      ("dtype", np.zeros((1, 70), np.float64)), ("int", np.zeros((1, 70), np.int32)), ("width", np.zeros((1, 64), np.float32))):
        _write(vis, "bad_" + what, arr)
        _write(text, "bad_" + what, np.zeros((1, 70), np.float32))
        with pytest.raises(MLAHipError, match=re.escape(os.path.join(vis, "bad_" + what + ".npy"))):
            load_feature_tables(names + ["bad_" + what], text, vis)
    _write(text, "only_text", np.zeros((1, 70), np.float32))
    with pytest.raises(MLAHipError, match=re.escape(os.path.join(vis, "only_text.npy"))):
        load_feature_tables(names + ["only_text"], text, vis)
    # permutation: the identity without shuffle, else a function of (seed, epoch) alone
    assert torch.equal(epoch_permutation(11, False, 5, 3), torch.arange(11))
    p = epoch_permutation(11, True, 5, 3)
    assert torch.equal(p, epoch_permutation(11, True, 5, 3)) and sorted(p.tolist()) == list(range(11)) and p.dtype == torch.int64
    assert not torch.equal(p, epoch_permutation(11, True, 5, 4)) and not torch.equal(p, epoch_permutation(11, True, 6, 3))
    labels = list(range(11))
    assert len(CLIPFeatureBatcher(names, labels, 4, text, vis, device="cpu")) == 3
    assert len(CLIPFeatureBatcher(names, labels, 4, text, vis, drop_last=True, device="cpu")) == 2
    assert len(CLIPFeatureBatcher(names, labels, 11, text, vis, drop_last=True, device="cpu")) == 1
    with pytest.raises(MLAHipError, match="labels"):
        CLIPFeatureBatcher(names, labels[:-1], 4, text, vis, device="cpu")
    # the range check of the index, where it is produced
    from mla_hip import ops
    ops.gather_index_check(torch.arange(11), 11)
    with pytest.raises(MLAHipError, match="outside"):
        ops.gather_index_check(torch.tensor([0, 11]), 11)
