"""CPU: the host side of Modal3Classifier(..., present=) -- Modal3Batcher.present, the validation of `present`, the row plans
and the three row ops' registration and argument checks (nothing here launches a kernel)."""
import numpy as np
import pytest
import torch


class _Args:
    fusion_method, dataset, gs_flag, modulation = "concat", "IEMOCAP", True, "Normal"


def test_batcher_present_is_the_mask_rows_of_each_batch(tmp_path):
    from mla_hip import Modal3Batcher
    from mla_hip.data import batch_ids
    n, bs = 7, 3
    mask = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 0], [0, 0, 1], [1, 1, 0], [0, 1, 0], [1, 0, 1]])
    names = [f"s{i}" for i in range(n)]
    for drop_last in (False, True):
        mb = Modal3Batcher(names, [0] * n, bs, str(tmp_path), audio_feature_path=str(tmp_path), visual_feature_path=str(tmp_path),
                           mask=mask, drop_last=drop_last, threads=1)
        try:
            batches = batch_ids(n, bs, drop_last)
            assert len(mb) == len(batches) == (2 if drop_last else 3)
            for step, ids in enumerate(batches):
                p = mb.present(step)
                assert p.dtype == torch.bool and p.device.type == "cpu" and tuple(p.shape) == (len(ids), 3)
                assert np.array_equal(p.numpy(), mask[list(ids)] != 0)
            with pytest.raises(IndexError):
                mb.present(len(batches))
        finally:
            mb.close()


def test_present_is_validated_before_anything_runs():
    from mla_hip import MLAHipError, Modal3Classifier
    model = Modal3Classifier(_Args(), device="cpu", depth=1, text_vocab_size=8, seed=0)
    B = 3
    token, pm = torch.zeros(B, 1, 256, dtype=torch.int64), torch.zeros(B, 1, 256)
    image, spec = torch.zeros(B, 3, 256, 256), torch.zeros(B, 1024, 128)
    ok = torch.tensor([[1, 1, 0], [0, 1, 1], [1, 0, 0]], dtype=torch.bool)
    for entry in (model.forward_split, model.forward_raw, model.forward):
        with pytest.raises(MLAHipError, match="HOST tensor"):
            entry(token, pm, image, spec, present=ok.to("meta"))             # stands for any device: it is not host memory
        with pytest.raises(MLAHipError, match="shape"):
            entry(token, pm, image, spec, present=ok[:2])
        with pytest.raises(MLAHipError, match="shape"):
            entry(token, pm, image, spec, present=ok.t().contiguous()[:, :2])
        with pytest.raises(MLAHipError, match="no modality"):
            entry(token, pm, image, spec, present=torch.tensor([[1, 1, 1], [0, 0, 0], [1, 0, 0]], dtype=torch.uint8))
        with pytest.raises(MLAHipError, match="dtype"):
            entry(token, pm, image, spec, present=ok.float())
        with pytest.raises(MLAHipError):
            entry(token, pm, image, spec, present=ok.tolist())
    runs = model.forward_split(token, pm, image, spec, present=ok)           # valid: three closures, nothing launched yet
    assert len(runs) == 3 and all(callable(r) for r in runs)
    from mla_hip import M3AEClassifier

    class A2(_Args):
        dataset = "MVSA"
    with pytest.raises(TypeError):                                           # the two-modality classifiers do not take it
        M3AEClassifier(A2(), device="cpu", depth=1, text_vocab_size=8, seed=0).forward_split(token, pm, image, present=ok[:, :2])


def test_row_plan_tables():
    from mla_hip.rows import RowPlan
    plan = RowPlan(torch.tensor([False, True, True, False, True]))
    assert (plan.B, plan.P, plan.A, plan.rows) == (5, 3, 2, 4)
    assert plan.idx_host.tolist() == [1, 2, 4] and plan.absent_host.tolist() == [0, 3]
    assert plan.map_host.tolist() == [3, 0, 1, 3, 2]                         # absent samples read row P: the zero row's feature
    none = RowPlan(torch.tensor([False, False]))
    assert (none.P, none.rows) == (0, 1) and none.map_host.tolist() == [0, 0]
    dev = torch.empty(10, dtype=torch.int64)
    plan.upload(dev)
    assert dev.tolist() == [1, 2, 4, 0, 3, 3, 0, 1, 3, 2]
    assert plan.idx.tolist() == [1, 2, 4] and plan.absent.tolist() == [0, 3] and plan.map.tolist() == plan.map_host.tolist()


def test_row_ops_are_registered_and_reject_bad_arguments_before_launch():
    """As test_cav_cpu.py::test_adam_step_rejects_bad_arguments_before_launch: fake (non-null, aligned, never dereferenced) device
    pointers, real host tables; every call must come back as MLA_ERR_INVALID_ARG with the function named in mla_last_error()."""
    from mla_hip import _lib
    lib = _lib.load()
    fake, fake2 = 0x1000, 0x100000
    idx = torch.tensor([4, 0], dtype=torch.int64)
    ih = idx.data_ptr()

    def rejected(fn, *args):
        assert getattr(lib, fn)(*args) == -1, f"{fn}{args} was not rejected"
        assert fn.encode() in lib.mla_last_error(), (fn, lib.mla_last_error())
    gather = lambda src, i, h, dst, B, P, row, eb, tail: rejected("mla_rows_gather", src, i, h, dst, B, P, row, eb, tail, None)
    gather(None, fake, ih, fake2, 5, 2, 64, 4, 1)                            # null pointers
    gather(fake, None, ih, fake2, 5, 2, 64, 4, 1)
    gather(fake, fake, None, fake2, 5, 2, 64, 4, 1)
    gather(fake, fake, ih, None, 5, 2, 64, 4, 1)
    gather(fake, fake, ih, fake2, 5, -1, 64, 4, 1)                           # P outside [0, B]
    gather(fake, fake, ih, fake2, 1, 2, 64, 4, 1)
    gather(fake, fake, ih, fake2, 0, 0, 64, 4, 1)                            # zero sizes
    gather(fake, fake, ih, fake2, 5, 2, 0, 4, 1)
    gather(fake, fake, ih, fake2, 5, 0, 64, 4, 0)                            # no destination row
    gather(fake, fake, ih, fake2, 5, 2, 64, 2, 1)                            # 2-byte elements
    gather(fake, fake, ih, fake2, 5, 2, 64, 4, -1)
    gather(fake + 2, fake, ih, fake2, 5, 2, 64, 4, 1)                        # misaligned
    gather(fake, fake, ih, fake2, 4, 2, 64, 4, 1)                            # idx[0] = 4 is outside [0, 4)
    assert b"idx[0] = 4" in lib.mla_last_error()
    gather(fake, fake, ih, fake + 256, 5, 2, 64, 4, 1)                       # dst inside src
    m = torch.tensor([2, 0, 1, 2, 3], dtype=torch.int64)
    expand = lambda src, mp, h, dst, B, S, row, eb: rejected("mla_rows_expand", src, mp, h, dst, B, S, row, eb, None)
    expand(None, fake, m.data_ptr(), fake2, 5, 4, 768, 4)
    expand(fake, fake, None, fake2, 5, 4, 768, 4)
    expand(fake, fake, m.data_ptr(), fake2, 0, 4, 768, 4)
    expand(fake, fake, m.data_ptr(), fake2, 5, 0, 768, 4)
    expand(fake, fake, m.data_ptr(), fake2, 5, 4, 0, 4)
    expand(fake, fake, m.data_ptr(), fake2, 5, 3, 768, 4)                    # map[4] = 3 is outside the 3 source rows
    assert b"map[4] = 3" in lib.mla_last_error()
    a = torch.tensor([1, 9], dtype=torch.int64)
    csum = lambda src, i, h, ab, ah, dst, B, P, A, row: rejected("mla_rows_compact_sum", src, i, h, ab, ah, dst, B, P, A, row, None)
    csum(None, fake, ih, fake, a.data_ptr(), fake2, 10, 2, 2, 768)
    csum(fake, fake, ih, fake, None, fake2, 10, 2, 2, 768)
    csum(fake, fake, ih, fake, a.data_ptr(), fake2, 10, 11, 2, 768)          # P > B
    csum(fake, fake, ih, fake, a.data_ptr(), fake2, 10, 2, -1, 768)
    csum(fake, fake, ih, fake, a.data_ptr(), fake2, 10, 2, 2, 0)
    csum(fake, fake, ih, fake, a.data_ptr(), fake2, 9, 2, 2, 768)            # absent_idx[1] = 9 is outside [0, 9)
    assert b"absent_idx[1] = 9" in lib.mla_last_error()
    import mla_hip.torch_ops as T
    for name in ("rows_gather", "rows_expand", "rows_compact_sum"):
        assert hasattr(torch.ops.mla_hip, name) and name in T.op_names()
    z = torch.zeros(4, 4)
    with pytest.raises(Exception):                                           # no CPU implementation: torch's "no kernel" error
        torch.ops.mla_hip.rows_gather(z, torch.tensor([0]), 1)
    with pytest.raises(Exception):
        torch.ops.mla_hip.rows_expand(z, torch.tensor([0]), 1, 4)
    with pytest.raises(Exception):
        torch.ops.mla_hip.rows_compact_sum(z, torch.tensor([0]), torch.tensor([1]))
