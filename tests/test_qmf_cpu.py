"""CPU: the QMF joint step's test model (tests/qmf_model.py) against the reference's outputs (tests/golden/qmf_small.npz,
make_golden_qmf.py), the conditions the fixture has to meet so that no comparison hangs on a rounding flip, the duplicate-index rule,
the new C-ABI entries, and the host side of mla_hip.qmf (heads, state_dict, guards)."""
import os

import numpy as np
import pytest
import torch

import qmf_model as Q
from oracle import mla_oracle as O


class AVArgs:
    fusion_method, dataset, gs_flag, modulation = "concat", "CREMAD", False, "Normal"


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "qmf_small.npz"))


@pytest.mark.parametrize("form", list(Q.FORMS))
@pytest.mark.parametrize("shape", Q.HEAD_CASES, ids=lambda s: "_".join(map(str, s)))
def test_model_reproduces_the_reference(fx, shape, form):
    """fp64 model against the reference's fp32 outputs: 1e-5 relative to each tensor's largest element; targets exact."""
    M, B, D, C, n_data = shape
    tag = Q.case_tag(shape, form)
    seed = int(fx[tag + ".seed"])
    hists = [Q.History(n_data) for _ in range(M)]
    Ws, bs = Q.head_inputs(O, seed, M, B, D, C)[1:]
    for s in range(3):
        p = f"{tag}.s{s}."
        xs = Q.head_inputs(O, seed + s, M, B, D, C)[0]
        assert np.array_equal(fx[p + "label"], O.portable_labels(seed + s, B, C).numpy())
        r = Q.qmf_step(xs, Ws, bs, fx[p + "label"], fx[p + "idx"], hists, *Q.FORMS[form])
        assert np.array_equal(r["target"].numpy(), fx[p + "target"].astype(np.float64)), p + "target"
        for k in ("z", "out", "conf", "ell", "margin", "ce", "rank", "cml", "loss"):
            Q.fixture_close(fx, p + k, r[k], 1e-5)
        for k in ("dW", "db", "dX"):
            Q.fixture_close(fx, p + k, torch.stack(r[k]), 1e-5)
        nz = fx[p + "hist_idx"]
        corr = np.stack([h.correctness for h in hists])
        assert set(np.nonzero(corr.any(axis=0))[0].tolist()) == set(nz.tolist())
        Q.fixture_close(fx, p + "hist_correctness", corr[:, nz], 1e-5)
        Q.fixture_close(fx, p + "hist_confidence", np.stack([h.confidence for h in hists])[:, nz], 1e-5)


@pytest.mark.parametrize("form", list(Q.FORMS))
@pytest.mark.parametrize("shape", Q.HEAD_CASES, ids=lambda s: "_".join(map(str, s)))
def test_fixture_input_conditions(fx, shape, form):
    """Asserted on the reference's own records.  Over the three steps of a case: every target value occurs, the hinge is active and
    inactive, every non-zero margin and every hinge argument t (c_i - r_i) of a pair with t != 0 is more than 1e-4 from its decision.
    A pair with t = 0 has margin 0 and hinge argument exactly 0 on every implementation: nothing there can flip.  The B = 1 case
    pairs the sample with itself, so its targets are all 0 and only the margin conditions apply to it."""
    tag = Q.case_tag(shape, form)
    t = np.concatenate([fx[f"{tag}.s{s}.target"].reshape(-1) for s in range(3)])
    mg = np.concatenate([fx[f"{tag}.s{s}.margin"].reshape(-1) for s in range(3)])
    ha = np.concatenate([fx[f"{tag}.s{s}.hinge_arg"].reshape(-1) for s in range(3)])
    assert np.isfinite(mg).all() and np.isfinite(ha).all()
    assert (mg[mg != 0] > 1e-4).all()
    assert (np.abs(ha[t != 0]) > 1e-4).all()
    assert (mg[t == 0] == 0).all() and (ha[t == 0] == 0).all()
    if shape[1] > 1:
        for v in (-1.0, 0.0, 1.0):
            assert (t == v).any(), f"target {v} never occurs"
        assert (ha > 0).any() and (ha[t != 0] < 0).any()
    else:
        assert (t == 0).all()


def test_duplicate_index_rule_equals_numpy():
    idx = np.array([4, 1, 4, 2, 1, 4, 0])
    ell = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5])
    conf = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7])
    h = Q.History(6)
    h.correctness[:] = np.arange(6) * 10.0
    want_corr, want_conf = h.correctness.copy(), h.confidence.copy()
    want_corr[idx] += ell                      # numpy's buffered fancy-index +=: the last occurrence wins
    want_conf[idx] = conf
    h.update(idx, ell, conf)
    assert np.array_equal(h.correctness, want_corr) and np.array_equal(h.confidence, want_conf)
    assert h.correctness[4] == 40.0 + 5.5 and h.correctness[1] == 10.0 + 4.5


def test_header_ctypes_and_library_agree_on_the_qmf_entries():
    from test_abi import header_functions
    from mla_hip import _lib
    lib = _lib.load()
    fns = header_functions()
    for name, n_args in (("mla_qmf_head_ws_elems", 3), ("mla_qmf_head_fwd_bwd", 39), ("mla_qmf_head_fwd", 17)):
        assert name in fns and len(fns[name]) == n_args == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(lib, name)
    assert lib.mla_abi_version() == 3                                   # additive change
    assert lib.mla_qmf_head_ws_elems(64, 6, 2) >= 2 * 2 * 64 * 6 + 64 * 6 + 64 + 2 * 64
    # argument checks come back as errors before any launch (pointers are never dereferenced)
    assert lib.mla_qmf_head_fwd(*([0x1000] * 12), 4, 2, 512, 6, None) == -1 and b"M must be" in lib.mla_last_error()
    assert lib.mla_qmf_head_fwd(*([0x1000] * 12), 2, 2, 512, 129, None) == -1
    assert lib.mla_qmf_head_fwd(0x1000, None, *([0x1000] * 10), 2, 2, 512, 6, None) == -1 and b"null" in lib.mla_last_error()


def test_attach_qmf_heads_state_dict(fx):
    from mla_hip import AVClassifier, attach_qmf_heads
    keys = [str(k) for k in fx["state_keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",") if d) for s in fx["state_shapes"]]
    m = AVClassifier(AVArgs(), device="cpu", seed=0)
    plain_keys = list(m.state_dict().keys())
    heads = attach_qmf_heads(m, seed=3)
    assert attach_qmf_heads(m) is heads and len(heads) == 2
    sd = m.state_dict(prefix="module.")
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert [k for k in m.state_dict() if k not in plain_keys] == ["audio_fc.weight", "audio_fc.bias", "visual_fc.weight", "visual_fc.bias"]
    m2 = AVClassifier(AVArgs(), device="cpu", seed=1)
    attach_qmf_heads(m2, seed=9)
    assert not torch.equal(m2.audio_fc.weight, m.audio_fc.weight)
    m2.load_state_dict(sd)                                              # `module.` prefix accepted
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd["module." + k]), k
    m2.load_state_dict(m.state_dict())
    # weight_init (utils/utils.py:106-114) reaches the new heads: they are nn.Linear
    from mla_hip import weight_init
    m2.audio_fc.bias.data.fill_(1.0)
    m2.apply(weight_init)
    assert float(m2.audio_fc.bias.detach().abs().max()) == 0.0


def test_modal3_gets_three_heads():
    from mla_hip import Modal3Classifier, attach_qmf_heads

    class A:
        fusion_method, dataset, gs_flag, modulation = "concat", "IEMOCAP", False, "Normal"
    m = Modal3Classifier(A(), device="cpu", depth=1, text_vocab_size=64, seed=0)
    attach_qmf_heads(m, seed=0)
    tail = list(m.state_dict().keys())[-6:]
    assert tail == ["audio_fc.weight", "audio_fc.bias", "visual_fc.weight", "visual_fc.bias", "txtual_fc.weight", "txtual_fc.bias"]
    assert m.txtual_fc.weight.shape == (4, 768)


def test_guards():
    from mla_hip import AVClassifier, Comm, QMFEvaluator, QMFTrainer, attach_qmf_heads
    from mla_hip._lib import MLAHipError
    comm = Comm()
    comm.world = 2                                                      # a two-rank communicator
    with pytest.raises(NotImplementedError, match="single-process"):
        QMFTrainer(AVClassifier(AVArgs(), device="cpu", seed=0), 10, comm=comm)

    class GS(AVArgs):
        gs_flag = True
    with pytest.raises(MLAHipError, match="gs_flag"):
        attach_qmf_heads(AVClassifier(GS(), device="cpu", seed=0))
    with pytest.raises(MLAHipError, match="attached"):
        QMFEvaluator(AVClassifier(AVArgs(), device="cpu", seed=0))


def test_unattached_model_is_unchanged():
    """An unattached AVClassifier still returns (a, v, out): its forward hands the features to the fusion module (stubbed here, as are
    the encoders: the kernels need a GPU)."""
    from mla_hip import AVClassifier
    m = AVClassifier(AVArgs(), device="cpu", seed=0)
    assert m.qmf_heads is None and not hasattr(m, "audio_fc")
    seen = {}
    m._calls = lambda *a: (2, [lambda out=None: out.fill_(0.0), lambda out=None: out.fill_(1.0)])
    m.fusion_module.forward = lambda a, v: seen.setdefault("res", (a, v, "out"))
    with torch.no_grad():
        res = m(torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 1, 8, 8))
    assert len(res) == 3 and res[2] == "out" and torch.equal(res[1], torch.ones(2, 512))
