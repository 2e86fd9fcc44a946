"""Modal3Classifier(..., present=): each encoder on the rows that have its modality plus one zero row, against the same step on all
rows of the same zero-filled inputs.

In exact arithmetic the two are one computation (no BatchNorm, no dropout: a sample's feature depends on its own row); they differ in
the order of floating-point sums, like two data-parallel ranks against one process on the whole batch.  The bound is the constant
tests/test_dist_gpu.py holds the transformer classifiers to in that comparison (test_two_rank_protocol_path_equals_global_batch:
`assert_close(r0["head"], ..., atol=1e-6, ...)`, and the two encoder lines beside it), applied to the features, the three losses, the
head and each encoder's flat parameters after two steps.  Smallest Modal3Classifier of test_m3ae_gpu.py (depth 2, vocabulary 200).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from util import assert_close  # noqa: E402

ATOL = 1e-6                  # tests/test_dist_gpu.py: the atol of its split-batch-against-whole-batch comparisons of transformer parameters
DEPTH, VOCAB, B, SEED = 2, 200, 5, 311
TAGS = ("a", "v", "t")

# columns (audio, image, text)
MASKS = {
    "all_present": [[1, 1, 1]] * 5,
    "one_modality_absent": [[1, 0, 1]] * 5,
    "mixed": [[0, 1, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1], [0, 0, 1]],       # first and last row absent, another pattern per modality
    "one_absent_row_each": [[1, 1, 0], [1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 1]],
}


class _Args:
    fusion_method, dataset, gs_flag, modulation = "concat", "IEMOCAP", True, "Normal"


def _inputs(mask):
    """(token, pm, image, spec) on the device with the rows of absent modalities zero, as Modal3Batcher leaves them, and the labels."""
    m = torch.tensor(mask)
    token = torch.from_numpy(np.minimum((O.portable_uniform(SEED, B * 256, 7) * VOCAB).astype(np.int64), VOCAB - 1)).view(B, 1, 256)
    pm = torch.zeros(B, 1, 256)
    for b in range(B):
        pm[b, 0, 40 + 37 * b:] = 1.0
    image = O.portable_normal(SEED, (B, 3, 256, 256), stream=3)
    spec = O.portable_normal(SEED, (B, 1024, 128), stream=4, mean=-5.081, std=4.4849)
    token, pm = token * m[:, 2].view(B, 1, 1), pm * m[:, 2].view(B, 1, 1)
    image, spec = image * m[:, 1].view(B, 1, 1, 1), spec * m[:, 0].view(B, 1, 1)
    return [x.cuda() for x in (token, pm, image, spec)], O.portable_labels(SEED, B, 4).cuda()


def _model():
    from mla_hip import Modal3Classifier
    return Modal3Classifier(_Args(), depth=DEPTH, text_vocab_size=VOCAB, seed=5)


def _two_steps(mask, with_present, overlap=True):
    from mla_hip import MLATrainer
    model = _model()
    tr = MLATrainer(model)
    tr.set_overlap(overlap)
    inputs, label = _inputs(mask)
    kw = {"present": torch.tensor(mask, dtype=torch.bool)} if with_present else {}
    res = {}
    for step in range(2):                                   # the second step: the projection has fired, the head has moved
        losses = tr.train_step(*inputs, label, step, 10, **kw)
        tr.join()
        torch.cuda.synchronize()
        for t in TAGS:
            res[f"feat_{t}{step}"] = tr.last[t].clone()
            res[f"out_{t}{step}"] = tr.last["out_" + t].clone()
            res[f"loss_{t}{step}"] = losses["loss_" + t].clone()
        res[f"loss{step}"] = losses["loss"].clone()
    res["head"] = model.fusion_module.fc_out.flat.clone()
    res["Pl"] = tr.gs_plugin.Pl.clone()
    for t, grp, enc in model.mla_encoders():
        res["enc_" + t] = enc.flat.clone()
        res["mom_" + t] = tr.optimizer.buf[grp].clone()
    res["mom_head"] = tr.optimizer.buf["head"].clone()
    return res


_cache = {}


def _pair(name, overlap=True):
    key = (name, overlap)
    if key not in _cache:
        _cache[key] = (_two_steps(MASKS[name], True, overlap), _two_steps(MASKS[name], False, overlap))
    return _cache[key]


def test_all_present_is_the_same_path_bit_for_bit():
    got, want = _pair("all_present")
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("name,overlap", [("one_modality_absent", True), ("mixed", True), ("mixed", False), ("one_absent_row_each", True)])
def test_two_steps_equal_the_step_on_all_rows(name, overlap):
    got, want = _pair(name, overlap)
    errs = {k: (got[k].double() - want[k].double()).abs().max().item() for k in want}
    print(f"\n[{name}, overlap={overlap}] max |present - all rows|: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for step in range(2):
        for t in TAGS:
            assert_close(got[f"feat_{t}{step}"], want[f"feat_{t}{step}"], atol=ATOL, name=f"features {t}, step {step}")
            assert_close(got[f"loss_{t}{step}"], want[f"loss_{t}{step}"], atol=ATOL, name=f"loss {t}, step {step}")
    assert_close(got["head"], want["head"], atol=ATOL, name="head after two steps")
    for t in TAGS:
        assert_close(got["enc_" + t], want["enc_" + t], atol=ATOL, name=f"encoder {t} parameters after two steps")
    # within the run with `present`, every absent sample of a modality has ONE feature: f(0), moved, not recomputed
    mask = torch.tensor(MASKS[name])
    for k, t in enumerate(TAGS):
        rows = torch.nonzero(mask[:, k] == 0).reshape(-1).tolist()
        for step in range(2):
            f = got[f"feat_{t}{step}"]
            for r in rows[1:]:
                assert torch.equal(f[r], f[rows[0]]), (t, step, r)


def test_evaluator_with_present_counts_the_same():
    from mla_hip import Evaluator
    mask = MASKS["mixed"]
    inputs, label = _inputs(mask)
    ev_p, ev_all = Evaluator(_model(), dynamic=True), Evaluator(_model(), dynamic=True)
    outs_p = ev_p.update(*inputs, label, present=torch.tensor(mask, dtype=torch.uint8))
    outs_all = ev_all.update(*inputs, label)
    torch.cuda.synchronize()
    for t, a, b in zip(TAGS, outs_p, outs_all):
        print(f"\nlogits {t}: max |present - all rows| = {(a.double() - b.double()).abs().max().item():.2e}")
        assert_close(a, b, atol=ATOL, name=f"logits {t}")
    assert torch.equal(ev_p.counts, ev_all.counts) and int(ev_p.counts[:4].sum()) == B
    assert ev_p.result() == ev_all.result()


def _protocol_two_steps(mask, with_present):
    """The reference's loop (main.py:424-470, three modalities) on the object protocol, as tests/test_dist_gpu.py::_protocol_steps."""
    import mla_hip
    model = mla_hip.DataParallel(_model())
    optimizer = mla_hip.FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    gs, criterion = mla_hip.GSPlugin(mode="as_published"), mla_hip.CrossEntropyLoss()
    inputs, label = _inputs(mask)
    kw = {"present": torch.tensor(mask, dtype=torch.bool)} if with_present else {}
    model.train()
    losses = []
    for batch_step in range(2):
        optimizer.zero_grad()
        feats = model(*inputs, **kw)
        for f in feats:
            out = model.module.fusion_module.fc_out(f)
            loss = criterion(out, label)
            loss.backward()
            gs.before_update(model.module.fusion_module.fc_out, f, batch_step, 10, gs.exp_count)
            optimizer.step()
            optimizer.zero_grad()
            gs.exp_count += 1
            losses.append(loss.detach().clone())
        for _n, p in model.named_parameters():
            if p.grad is not None:
                del p.grad
    torch.cuda.synchronize()
    m = model.module
    res = {"losses": torch.stack(losses), "head": m.fusion_module.fc_out.flat.clone()}
    res.update({"enc_" + t: enc.flat.clone() for t, _g, enc in m.mla_encoders()})
    return res


def test_protocol_path_with_present():
    got, want = _protocol_two_steps(MASKS["mixed"], True), _protocol_two_steps(MASKS["mixed"], False)
    print("\n[protocol, mixed] max |present - all rows|: " + ", ".join(f"{k}={(got[k].double() - want[k].double()).abs().max().item():.2e}" for k in want))
    for k in want:
        assert_close(got[k], want[k], atol=ATOL, name=f"protocol path: {k}")


def _ptrs(enc):
    return {path: t.data_ptr() for path, t in enc.workspace_tensors().items()}


def _unmoved(enc, planned):
    now = _ptrs(enc)
    return all(now.get(path) == ptr for path, ptr in planned.items())


@pytest.mark.parametrize("kind", ["text", "image", "audio"])
def test_workspace_is_planned_once(kind):
    """Steps on P + 1 = 3, 6 and 2 rows of one encoder run in ONE allocation: after reserve(6) nothing of it moves, and without a
    reservation only the step to more rows than any before allocates."""
    from mla_hip import M3AEEncoder

    def step(enc, rows):
        if kind == "text":
            enc.forward(torch.zeros(rows, 1, 256, dtype=torch.int64, device="cuda"), torch.zeros(rows, 1, 256, device="cuda"))
        else:
            enc.forward(torch.zeros((rows, 3, 256, 256) if kind == "image" else (rows, 1024, 128), device="cuda"))
        enc.backward_from_pooled(torch.ones(rows, 768, device="cuda"))
        assert enc._ws["B"] == rows and enc._ws["x0"].shape[0] == rows * enc._ws["n"]
    L = {"text": 256, "image": 256, "audio": 512}[kind]
    enc = M3AEEncoder(kind, depth=DEPTH, text_vocab_size=VOCAB, seed=1)
    enc.reserve(6, L)
    planned = _ptrs(enc)
    assert len(planned) > 10 * DEPTH
    for rows in (3, 6, 2):
        step(enc, rows)
        assert _unmoved(enc, planned), rows
    enc = M3AEEncoder(kind, depth=DEPTH, text_vocab_size=VOCAB, seed=1)
    step(enc, 3)
    step(enc, 6)                                             # more rows than any before: the one reallocation
    planned = _ptrs(enc)
    for rows in (2, 3, 6):
        step(enc, rows)
        assert _unmoved(enc, planned), rows
    torch.cuda.synchronize()


def test_full_batch_call_after_present_calls_is_unchanged():
    """A model that has run with `present` (smaller row counts, prefix views of its workspace) then runs a call on all rows exactly
    as a fresh model does: features and a whole training step bit for bit."""
    from mla_hip import MLATrainer
    mask = MASKS["mixed"]
    inputs, label = _inputs(mask)
    used, fresh = _model(), _model()
    used.eval()
    used.forward_raw(*inputs, present=torch.tensor(mask, dtype=torch.bool))
    used.forward_raw(*inputs, present=torch.tensor(MASKS["one_absent_row_each"], dtype=torch.bool))
    fresh.eval()
    for a, b in zip(used.forward_raw(*inputs), fresh.forward_raw(*inputs)):
        assert torch.equal(a, b)
    res = []
    for model in (used, fresh):
        tr = MLATrainer(model)
        losses = tr.train_step(*inputs, label, 0, 10)
        tr.join()
        torch.cuda.synchronize()
        res.append([losses[k].clone() for k in sorted(losses)] + [model.fusion_module.fc_out.flat.clone()]
                   + [enc.flat.clone() for _t, _g, enc in model.mla_encoders()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
