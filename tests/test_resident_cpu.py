"""CPU: the host side of the HBM-resident CREMA-D feed (mla_hip/resident_feed.py, csrc/resident_args.h): the restatement of the
device draw (tests/resident_model.py) pinned and checked for its properties and its distribution, the plan against the library's,
the refusals of mla_resident_plan / mla_resident_batch through the C ABI (which launch nothing, so they need no GPU), the host
sanitizer check, and ResidentStore's size refusal."""
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import resident_model as M
from mla_hip import MLAHipError, _lib, frames, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(36, 48), (50, 40), (360, 480), (8, 200)]


def test_philox_restatement_known_answer():
    """Random123's known-answer vectors for philox4x32-10."""
    ff = 0xFFFFFFFFFFFFFFFF
    assert M.philox4x32_10(ff, ff, ff) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert M.philox4x32_10(0, 0, 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # pi digits: counter 243f6a8885a308d3 13198a2e03707344, key a4093822 299f31d0
    assert M.philox4x32_10(0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_literals_are_the_logs():
    assert M.L0 == math.log(3 / 4) and M.L1 == math.log(4 / 3)
    src = open(os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd", "csrc", "resident_args.h")).read()
    assert "-0x1.269621134db92p-2" in src and "0x1.269621134db91p-2" in src          # the header holds the same literals


def _fixed_draws(n):
    """n (shape, seed, epoch, index, t) tuples, fixed."""
    rng = np.random.default_rng(2024)
    return [(SHAPES[q % len(SHAPES)], int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 40)),
             int(rng.integers(0, 3))) for q in range(n)]


def test_every_box_lies_inside_its_frame_and_the_fallback_is_reached():
    fell = {s: 0 for s in SHAPES}
    flips = 0
    draws = _fixed_draws(4000)
    for (H, W), seed, epoch, index, t in draws:
        (top, left, h, w, flip), tries, accepted, _ = M.draw(H, W, seed, epoch, index, t)
        assert 0 < h <= H and 0 < w <= W and 0 <= top <= H - h and 0 <= left <= W - w and flip in (0, 1)
        assert 1 <= tries <= 10 and (accepted or tries == 10)
        if not accepted:
            fell[(H, W)] += 1
            assert (top, left, h, w) == M.fallback(H, W)
        flips += flip
    print("fallbacks per shape", fell, "flips", flips)
    assert fell[(8, 200)] > 100                                   # 8 x 200 lies outside the ratio range: most tries are refused
    assert M.fallback(8, 200) == (0, 94, 8, 11) and M.fallback(200, 8) == (94, 0, 11, 8) and M.fallback(36, 48) == (0, 0, 36, 48)
    assert abs(flips - 2000) < 5 * math.sqrt(4000 * 0.25)


def test_a_draw_depends_on_seed_epoch_index_and_slot_only_and_on_each_of_them():
    base = M.draw(360, 480, 5, 7, 11, 1)
    assert M.draw(360, 480, 5, 7, 11, 1) == base
    others = [M.draw(360, 480, 6, 7, 11, 1), M.draw(360, 480, 5, 8, 11, 1), M.draw(360, 480, 5, 7, 12, 1), M.draw(360, 480, 5, 7, 11, 2),
              M.draw(360, 480, 7, 5, 11, 1)]                     # (seed, epoch) swapped: another key
    assert all(o[0] != base[0] for o in others)
    for bad in ((1 << 32, 0), (0, 1 << 32)):
        with pytest.raises(AssertionError):
            M.block(bad[0], bad[1], 0, 0, 0)


def gpu_draws():
    """Every draw tests/test_resident_gpu.py compares with the kernel's: (H, W, seed, epoch, index, t)."""
    return [(M.GPU_SIZES[i % 4] + (M.GPU_SEED, e, i, t)) for e in M.GPU_EPOCHS for i in range(M.GPU_N) for t in range(M.GPU_T)]


def test_margin_of_the_gpu_draws():
    """For every try of every draw the GPU tests compare, both roots are more than 1e-6 from a half-integer: one ulp between the
    device's fp64 exp / sqrt and the host's (about 1e-13 at these magnitudes) cannot move an integer."""
    worst = min(M.draw(*d)[3] for d in gpu_draws())
    print("least distance of a root from a half-integer:", worst)
    assert worst > 1e-6


def _rate(successes, trials):
    p = successes / trials
    return p, math.sqrt(p * (1 - p) / trials)


def test_distribution_equals_sample_crop_on_torch_generators(monkeypatch):
    """20 000 draws of the restatement against frames.sample_crop (torchvision's get_params on torch generators), shape by shape:
    the mean crop-area fraction and the acceptance rate per try agree within five standard errors of their difference (sample
    variances; the tries are independent Bernoulli trials).  sample_crop's tries are counted by its calls of math.sqrt, two each."""
    calls = [0]

    def counting_sqrt(x):
        calls[0] += 1
        return math.sqrt(x)
    monkeypatch.setattr(frames, "math", types.SimpleNamespace(sqrt=counting_sqrt))
    per = 20000 // len(SHAPES)
    for (H, W) in SHAPES:
        area_m, area_t, acc_m, acc_t, tries_m = [], [], 0, 0, 0
        calls[0] = 0
        for q in range(per):
            (_, _, h, w, _), tries, accepted, _ = M.draw(H, W, 17, 3, q, q % 3)
            area_m.append(h * w / (H * W))
            acc_m += accepted
            tries_m += tries
            box = frames.sample_crop(H, W, frames.sample_generator(17, 3, q))
            area_t.append(box[2] * box[3] / (H * W))
            acc_t += tuple(box) != M.fallback(H, W)
        tries_t = calls[0] // 2
        am, at = np.asarray(area_m), np.asarray(area_t)
        se = math.sqrt(am.var(ddof=1) / per + at.var(ddof=1) / per)
        (pm, sm), (pt, st) = _rate(acc_m, tries_m), _rate(acc_t, tries_t)
        print(f"{H}x{W}: mean area fraction {am.mean():.4f} vs {at.mean():.4f} (se {se:.4f}); acceptance per try {pm:.4f} of {tries_m} vs "
              f"{pt:.4f} of {tries_t} (se {math.hypot(sm, st):.4f})")
        assert abs(am.mean() - at.mean()) <= 5 * se
        assert abs(pm - pt) <= 5 * math.hypot(sm, st)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
def _table(shapes):
    rows, off = [], 0
    for H, W in shapes:
        rows.append((off, H, W))
        off += H * W * 3
    return torch.tensor(rows, dtype=torch.int64), off


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("out", [(40, 40), (224, 224), (17, 33)])
def test_plan_of_the_restatement_equals_the_librarys(out, train):
    for shapes in ([s] for s in SHAPES + [(90, 120)]):
        table, nbytes = _table(shapes)
        got = ops.resident_plan(table, 1, nbytes, out[0], out[1], train)
        assert tuple(got.plan5.tolist()) == M.plan(shapes, out[0], out[1], train), (shapes, out, train)
    shapes = SHAPES + [(90, 120), (36, 48)]
    table, nbytes = _table(shapes)
    got = ops.resident_plan(table, 3, nbytes, out[0], out[1], train)
    assert tuple(got.plan5.tolist()) == M.plan(shapes, out[0], out[1], train)
    assert got.train == train and (got.out_h, got.out_w) == out


def test_the_train_plan_covers_every_crop():
    """kh / kv / rows_cap of the train plan are at least what any single crop of the frame needs at the plan's band."""
    table, nbytes = _table([(90, 120)])
    band, rows_cap, kh, kv, _ = ops.resident_plan(table, 1, nbytes, 40, 40, True).plan5.tolist()
    for ch in range(1, 91):
        assert M.band_rows(ch, 40, band) <= rows_cap and M.ksize(ch, 40) <= kv
    assert all(M.ksize(cw, 40) <= kh for cw in range(1, 121))


# ---- refusals through the C ABI: none of them launches anything ----------------------------------------------------------------------
def test_plan_refusals_through_the_c_abi():
    lib = _lib.load()
    plan5 = torch.zeros(5, dtype=torch.int32)

    def call(rows, T, nbytes, out=(40, 40), train=1, count=None):
        t = torch.tensor(rows, dtype=torch.int64)
        return lib.mla_resident_plan(t.data_ptr(), t.shape[0] if count is None else count, T, nbytes, out[0], out[1], train, plan5.data_ptr())

    def refused(rc, text):
        assert rc == -1 and b"mla_resident_plan" in lib.mla_last_error() and text in lib.mla_last_error(), lib.mla_last_error()
    size = 36 * 48 * 3
    assert call([[0, 36, 48]], 1, size) == 0 and plan5[0] == 16
    refused(call([[1, 36, 48]], 1, size), b"lie outside")                               # a frame outside the buffer, by one byte
    refused(call([[0, 36, 48], [size, 36, 48]], 1, 2 * size - 1), b"lie outside")
    refused(call([[-1, 36, 48]], 1, size), b"lie outside")
    far = (5 << 32) + 7                                                                   # an offset above 2^32
    assert call([[far, 36, 48]], 1, far + size) == 0
    refused(call([[far, 36, 48]], 1, far + size - 1), b"lie outside")
    refused(call([[(1 << 63) - 1, 36, 48]], 1, size), b"lie outside")                    # offset + size would overflow
    refused(call([[0, 36, 48], [size, 36, 48]], 3, 2 * size), b"are not N * T rows")     # a wrong row count
    refused(call([[0, 36, 48]], 1, size, count=0), b"are not N * T rows")
    refused(call([[0, 0, 48]], 1, size), b"out of range")
    refused(call([[0, 36, 65537]], 1, 1 << 40), b"out of range")
    refused(call([[0, 36, 48]], 1, size, out=(0, 40)), b"output size")
    refused(call([[0, 65536, 2]], 1, 65536 * 6, out=(4, 4096), train=0), b"65536x2 frame")          # no band fits 64 KB: the size is named
    with pytest.raises(MLAHipError, match="frame table"):
        ops.resident_plan(torch.zeros((2, 8), dtype=torch.int64), 1, 100)


def test_batch_refusals_through_the_c_abi():
    lib = _lib.load()
    fake = 0x1000                                       # non-null, 16-byte aligned, never dereferenced: validation fails first
    good = ops.resident_plan(torch.tensor([[0, 36, 48]]), 1, 36 * 48 * 3, 40, 40, True).plan5

    def call(N=7, T=3, pos=0, b=3, seed=0, epoch=0, plan=good, out=(40, 40), spec=fake, spec_out=fake, table=fake, lut=fake, frames=fake):
        return lib.mla_resident_batch(frames, 1 << 20, table, spec, fake, fake, N, T, pos, b, seed, epoch, 1, plan.data_ptr(), lut, fake, fake,
                                      spec_out, fake, fake, out[0], out[1], None)

    def refused(rc, text):
        assert rc == -1 and b"mla_resident_batch" in lib.mla_last_error() and text in lib.mla_last_error(), lib.mla_last_error()
    refused(call(pos=5, b=3), b"leaves the order")                                       # pos + b > N
    refused(call(pos=7, b=1), b"leaves the order")
    refused(call(N=1 << 20, b=21846), b"max 65535")                                      # b * T = 65538
    refused(call(seed=1 << 32), b"below 2^32")
    refused(call(epoch=1 << 32), b"below 2^32")
    refused(call(seed=(1 << 64) - 1), b"below 2^32")
    refused(call(frames=None), b"null pointer")
    refused(call(spec_out=None), b"no spec_out")
    refused(call(table=fake + 4), b"8-byte aligned")
    refused(call(lut=fake + 2), b"4-byte aligned")
    refused(call(spec=fake + 8), b"16-byte aligned")
    for k, v, text in ((0, 12, b"band 12"), (0, 32, b"band 32"), (1, 0, b"rows_cap"), (2, 4, b"filter sizes"), (3, 1, b"filter sizes"),
                       (4, int(good[4]) - 16, b"bytes of LDS where"), (1, int(good[1]) + 1, b"bytes of LDS where"),
                       (1, 60000, b"bytes of LDS (max")):                                  # forged plans
        forged = good.clone()
        forged[k] = v
        refused(call(plan=forged), text)
    refused(call(out=(40, 48)), b"bytes of LDS where")                                   # the plan of another output width
    refused(call(out=(40, 5000)), b"output size")
    with pytest.raises(MLAHipError, match="do not match"):                               # the wrapper's own shape checks need no GPU either
        ops.resident_batch(torch.zeros(4, dtype=torch.uint8), torch.zeros((3, 3), dtype=torch.int64), None, torch.zeros(2, dtype=torch.int64),
                           torch.zeros(2, dtype=torch.int64), 3, 0, 1, 0, 0, True, ops.ResidentPlan(good, 40, 40, True), torch.zeros(3, 256),
                           None, None, None, None, None)
    assert lib.mla_abi_version() == 3


def test_host_check_builds_and_runs_under_the_host_sanitizers():
    """`make host-check` builds resident_host_check (a stand-alone program; nothing is preloaded) with
    -fsanitize=address,undefined and runs it with the other host checks."""
    csrc = os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "host-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resident host check ok" in r.stdout and "-fsanitize=address,undefined" in r.stdout


# ---- the store's host half -----------------------------------------------------------------------------------------------------------
def _cache(root, sizes, T=3):
    names = [f"clip{i}" for i in range(len(sizes))]
    for name, (H, W) in zip(names, sizes):
        os.makedirs(os.path.join(root, name))
        for t in range(T):
            np.save(os.path.join(root, name, f"{t}.npy"), np.full((H, W, 3), t, dtype=np.uint8))
    return names


def test_frame_table_packs_back_to_back_in_decode_frames_order(tmp_path):
    from mla_hip import frame_table
    sizes = [(36, 48), (50, 40), (8, 200)]
    names = _cache(str(tmp_path), sizes)
    table, nbytes, files = frame_table(names, frame_cache=str(tmp_path))
    assert table.dtype == torch.int64 and tuple(table.shape) == (9, 3)
    off = 0
    for i, (H, W) in enumerate(sizes):
        for t in range(3):
            assert table[i * 3 + t].tolist() == [off, H, W] and files[i][t].endswith(os.path.join(names[i], f"{t}.npy"))
            off += H * W * 3
    assert nbytes == off
    ops.resident_plan(table, 3, nbytes, 40, 40, True)                                     # and the library accepts it
    with pytest.raises(ValueError, match="exactly one of visual_feature_path"):
        frame_table(names)
    with pytest.raises(MLAHipError, match="cannot read"):
        frame_table(names + ["absent"], frame_cache=str(tmp_path))


def test_store_refuses_a_dataset_above_max_bytes_before_allocating(tmp_path, monkeypatch):
    from mla_hip import ResidentFrameBatcher, ResidentStore
    sizes = [(36, 48), (50, 40)]
    names = _cache(str(tmp_path), sizes)
    frames_bytes = 3 * 3 * (36 * 48 + 50 * 40)
    spec_bytes = 2 * 1024 * 128 * 4

    def no_allocation(*a, **k):
        raise AssertionError("the store allocated before it refused")
    monkeypatch.setattr(torch, "empty", no_allocation)
    with pytest.raises(MLAHipError, match=f"{frames_bytes} of frames, {spec_bytes} of spectrograms.*max_bytes = 1000"):
        ResidentStore(names, [0, 1], frame_cache=str(tmp_path), audio_feature_path="absent", max_bytes=1000)
    with pytest.raises(MLAHipError, match=f"{frames_bytes} of frames, 0 of spectrograms"):
        ResidentStore(names, [0, 1], frame_cache=str(tmp_path), max_bytes=frames_bytes)   # the tables count too
    with pytest.raises(MLAHipError, match="max_bytes = 1000"):
        ResidentFrameBatcher(names, [0, 1], 2, frame_cache=str(tmp_path), audio_feature_path="absent", max_bytes=1000)
    with pytest.raises(ValueError, match="exactly one of audio_feature_path"):
        ResidentFrameBatcher(names, [0, 1], 2, frame_cache=str(tmp_path))
    with pytest.raises(ValueError, match="exactly one of visual_feature_path"):
        ResidentStore(names, [0, 1], audio_feature_path="absent", max_bytes=1000)
    with pytest.raises(ValueError, match="at most one of audio_feature_path"):
        ResidentStore(names, [0, 1], frame_cache=str(tmp_path), audio_feature_path="a", audio_wav_path="b", max_bytes=1000)


def test_field_order_and_exports():
    import inspect
    import mla_hip
    from mla_hip import torch_ops
    for name in ("ResidentStore", "ResidentFrameBatcher", "frame_table"):
        assert hasattr(mla_hip, name)
    assert "resident_batch" in torch_ops.op_names()
    assert {"mla_resident_plan", "mla_resident_batch"} <= set(_lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES["mla_resident_plan"][1]) == 8 and len(_lib.PROTOTYPES["mla_resident_batch"][1]) == 23
    params = list(inspect.signature(mla_hip.ResidentFrameBatcher.__init__).parameters)
    assert params[1:4] == ["names", "labels", "batch_size"]
    for kw in ("store", "train", "shuffle", "seed", "drop_last", "out_size", "pick_num", "mean", "std", "depth"):
        assert inspect.signature(mla_hip.ResidentFrameBatcher.__init__).parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    doc = mla_hip.ResidentFrameBatcher.__doc__
    assert "(spec (b, 1024, 128), image (b, 3, T, out, out), label (b,), idx (b, 1))" in doc and "Slot contract" in doc
    assert ops.ResidentPlan._fields == ("plan5", "out_h", "out_w", "train")
    with pytest.raises(NotImplementedError):                                              # no CPU implementation, like the other feed ops
        torch.ops.mla_hip.resident_batch(torch.zeros(3, dtype=torch.uint8), torch.zeros((1, 3), dtype=torch.int64), None,
                                         torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 1, 0, 1, 0, 0, True,
                                         torch.zeros(3, 256))
