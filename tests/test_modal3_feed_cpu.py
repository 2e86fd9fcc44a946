"""CPU: the Modal3 batch feed's host side (mla_hip.modal3_feed) -- random_mask against the matrices the reference's function
returned (tests/golden/modal3_mask_small.npz, made by make_golden_modal3.py), the launch checks of mla_modal3_assemble, and
Modal3Batcher's host tuples: what a masked-out modality leaves out, and that it is never opened."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from mla_hip import (M3AEBatcher, MLAHipError, Modal3Batcher, decode_middle_frames, mask_descriptors, ops, pick_middle_frame,
                     random_mask)
from mla_hip.frames import decode_jpeg

OUT = 40
ALL_ROWS = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]]      # (audio, image, text): every non-zero row


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "modal3_mask_small.npz")))


def test_random_mask_equals_the_reference_matrices(fixture):
    n_cases = len(fixture["n"])
    assert n_cases == 2 * 7 * 3
    regimes = set()
    for k in range(n_cases):
        n, rate, seed = int(fixture["n"][k]), float(fixture["rate"][k]), int(fixture["seed"][k])
        got = random_mask(3, n, rate, np.random.RandomState(seed))
        assert got.dtype == np.int64 and got.shape == (n, 3)
        assert np.array_equal(got, fixture[f"mask_{k}"]), (n, rate, seed)
        assert (got.sum(axis=1) >= 1).all()
        if 1 - rate <= 1 / 3:
            assert (got.sum(axis=1) == 1).all()
            regimes.add("one")
        elif rate == 0:
            assert (got == 1).all()
            regimes.add("all")
        else:
            assert abs(got.mean() - (1 - rate)) < 0.005
            regimes.add("loop")
    assert regimes == {"one", "all", "loop"}


def test_random_mask_raises_where_the_tolerance_cannot_be_met():
    """n = 8 at rate 0.3: 24 entries, the nearest shares of ones 17/24 = 0.7083 and 16/24 = 0.6667 are both further than 0.005
    from 0.7, so no round can succeed whatever the cap."""
    assert min(abs(k / 24 - 0.7) for k in range(25)) > 0.005
    with pytest.raises(MLAHipError, match=r"8 x 3 .* 0\.005 .* 0\.3"):
        random_mask(3, 8, 0.3, np.random.RandomState(0), max_iter=50)


def test_mask_descriptors_slots_in_batch_order():
    d = mask_descriptors(np.array(ALL_ROWS))
    assert d.dtype == np.int64 and d[:, :3].tolist() == ALL_ROWS and d[:, 3].tolist() == [-1, 0, -1, 1, -1, 2, 3]
    assert mask_descriptors(np.array([[1, 0, 1]]))[:, 3].tolist() == [-1]


def _table(rows, slots):
    return torch.tensor([r + [s] for r, s in zip(rows, slots)], dtype=torch.int64)


OK_SLOTS = [-1, 2, -1, 0, -1, 3, 1]              # a permutation that is not in batch order


def test_modal3_assemble_check_accepts_and_refuses_tables_and_sizes():
    ok = _table(ALL_ROWS, OK_SLOTS)
    ops.modal3_assemble_check(ok, 4)
    ops.modal3_assemble_check(ok, 4, 36, 24 * 4, 12)
    ops.modal3_assemble_check(_table([[1, 0, 1], [0, 0, 1]], [-1, -1]), 0)            # no image at all

    def bad(row, col, val, match, P=4, **kw):
        t = ok.clone()
        if row is not None:
            t[row, col] = val
        with pytest.raises(MLAHipError, match=match):
            ops.modal3_assemble_check(t, P, **kw)
    bad(0, 0, 2, "not 0 or 1")
    bad(3, 1, -1, "not 0 or 1")
    bad(6, 2, 5, "not 0 or 1")
    bad(0, 3, 0, "has no image but slot 0")
    bad(1, 3, -1, r"outside \[0, 4\)")
    bad(1, 3, 4, r"outside \[0, 4\)")
    bad(1, 3, 3, "used twice")
    bad(None, None, None, "4 samples have an image but P=5", P=5)
    bad(None, None, None, r"outside \[0, 3\)", P=3)
    bad(None, None, None, "0 <= P <= B", P=8)
    bad(None, None, None, "0 <= P <= B", P=-1)
    bad(None, None, None, "multiples of 4", S=3)
    bad(None, None, None, "multiples of 4", TF=126)
    bad(None, None, None, "multiples of 4", L=6)
    bad(None, None, None, "> 0", S=0)
    bad(None, None, None, "> 0", TF=0)
    bad(None, None, None, "> 0", L=-4)
    with pytest.raises(MLAHipError, match=r"\(N, 4\)"):
        ops.modal3_assemble_check(ok[:, :3].contiguous(), 4)
    with pytest.raises(MLAHipError, match="int64"):
        ops.modal3_assemble_check(ok.int(), 4)


def test_modal3_assemble_refuses_bad_buffers_before_any_launch():
    """The C entry point validates before it launches: fake addresses, no GPU."""
    from mla_hip import _lib
    lib = _lib.load()
    t = _table(ALL_ROWS, OK_SLOTS).numpy()
    tp = t.ctypes.data_as(ctypes.c_void_p)
    B, P, S, TF, L = 7, 4, OUT, 64 * 16, 256
    img = 3 * S * S * 4
    compact, spec, token, pm, mdesc, out = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000

    def call(**kw):
        a = dict(compact=compact, spec=spec, token=token, pm=pm, mdesc=mdesc, host=tp, out=out, B=B, P=P, S=S, TF=TF, L=L)
        a.update(kw)
        return lib.mla_modal3_assemble(a["compact"], a["spec"], a["token"], a["pm"], a["mdesc"], a["host"], a["out"], a["B"], a["P"],
                                       a["S"], a["TF"], a["L"], None)
    for name in ("compact", "spec", "token", "pm", "mdesc", "host", "out"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.mla_last_error(), name
    for name in ("B", "S", "TF", "L"):
        assert call(**{name: 0}) == -1 and b"> 0" in lib.mla_last_error(), name
    assert call(S=37) == -1 and b"multiples of 4" in lib.mla_last_error()
    assert call(TF=1022) == -1 and b"multiples of 4" in lib.mla_last_error()
    assert call(L=254) == -1 and b"multiples of 4" in lib.mla_last_error()
    for name in ("compact", "spec", "token", "pm", "out"):
        assert call(**{name: 0x700008}) == -1 and b"16-byte aligned" in lib.mla_last_error(), name
    assert call(mdesc=0x500004) == -1 and b"8-byte aligned" in lib.mla_last_error()
    # image_out against each input: the last 16 bytes of one on the first 16 of the other, both ways
    for name, nbytes in (("compact", P * img), ("spec", B * TF * 4), ("token", B * L * 8), ("pm", B * L * 4), ("mdesc", B * 4 * 8)):
        base = dict(compact=compact, spec=spec, token=token, pm=pm, mdesc=mdesc)[name]
        assert call(out=base + nbytes - 16) == -1 and b"overlaps" in lib.mla_last_error(), name
        assert call(out=base - B * img + 16) == -1 and b"overlaps" in lib.mla_last_error(), name
    bad = t.copy()
    bad[1, 3] = 3
    assert call(host=bad.ctypes.data_as(ctypes.c_void_p)) == -1 and b"used twice" in lib.mla_last_error()
    assert call(P=3) == -1 and b"outside [0, 3)" in lib.mla_last_error()
    assert call(P=5) == -1 and b"P=5" in lib.mla_last_error()
    assert lib.mla_modal3_assemble_check(tp, B, P, S, TF, L) == 0


def _write_modal3_dataset(root, n_samples, sizes, seed=0, n_frames=3):
    """<root>/text, /audio, /visual/<name>/<frame>.jpg (Modal3Dataset's layout) and /flat/<name>.jpg, a copy of the frame the
    reference picks (M3AEDataset's layout, for M3AEBatcher on the same images)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(seed)
    text, audio, visual, flat = (os.path.join(root, d) for d in ("text", "audio", "visual", "flat"))
    for d in (text, audio, visual, flat):
        os.makedirs(d)
    names = [f"clip{i}" for i in range(n_samples)]
    for i, name in enumerate(names):
        n_tok = 5 + 3 * i
        token = np.zeros((1, 256), dtype=np.int64)
        token[0, :n_tok] = rng.integers(1, 64, n_tok)
        pm = np.ones((1, 256), dtype=np.float32)
        pm[0, :n_tok] = 0.0
        np.save(os.path.join(text, name + "_token.npy"), token)
        np.save(os.path.join(text, name + "_pm.npy"), pm)
        np.save(os.path.join(audio, name + ".npy"), (rng.standard_normal((1024, 128)) * 4.4849 - 5.081).astype(np.float32))
        H, W = sizes[i % len(sizes)]
        yy, xx = np.mgrid[0:H, 0:W]
        os.makedirs(os.path.join(visual, name))
        for t in range(n_frames):
            img = np.stack([(xx * 3 + i * 40 + t * 9) % 256, (yy * 2 + i * 30) % 256, (xx + yy + i * 17 + t * 50) % 256], -1).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(visual, name, f"frame_{t:04d}.jpg"), quality=90)
        d = os.path.join(visual, name)
        shutil.copyfile(os.path.join(d, pick_middle_frame(d)), os.path.join(flat, name + ".jpg"))
    return names, text, audio, visual, flat


def _delete_absent(mask, names, text, audio, visual):
    for m, name in zip(mask, names):
        if not m[0]:
            os.remove(os.path.join(audio, name + ".npy"))
        if not m[1]:
            shutil.rmtree(os.path.join(visual, name))
        if not m[2]:
            os.remove(os.path.join(text, name + "_token.npy"))
            os.remove(os.path.join(text, name + "_pm.npy"))


def _clone(fb):
    out = []
    try:
        for b in fb:
            nbytes = int(b[4][-1, 0] + b[4][-1, 1] * b[4][-1, 2] * 3) if b[4].shape[0] else 0
            out.append(tuple(t[:nbytes].clone() if k == 3 else t.clone() for k, t in enumerate(b)))
    finally:
        fb.close()
    return out


SIZES = [(60, 64), (48, 40), (64, 50)]


def test_modal3_batcher_host_tuples_and_untouched_absent_files(tmp_path):
    names, text, audio, visual, flat = _write_modal3_dataset(str(tmp_path), 7, SIZES)
    cache = str(tmp_path / "cache")
    assert decode_middle_frames(visual, cache, names, threads=3) == 7
    labels = [3, 2, 1, 0, 3, 2, 1]
    mask = np.array(ALL_ROWS)
    want_p, want_slots = [1, 2, 1], [[-1, 0, -1], [0, -1, 1], [0]]
    for train in (True, False):
        kw = dict(train=train, seed=4, pin=False, out_size=OUT, mask=mask)
        a = _clone(Modal3Batcher(names, labels, 3, text, audio, visual_feature_path=visual, threads=1, **kw))
        b = _clone(Modal3Batcher(names, labels, 3, text, audio, visual_feature_path=visual, threads=4, ring=2, **kw))
        c = _clone(Modal3Batcher(names, labels, 3, text, audio, frame_cache=cache, threads=1, **kw))
        # the image draws of a sample do not depend on its neighbours: M3AEBatcher on the same images, nothing masked
        m3b = M3AEBatcher(names, labels, 7, text, visual_feature_path=flat, train=train, seed=4, pin=False, out_size=OUT)
        m3 = [tuple(t.clone() for t in batch) for batch in m3b][0]
        m3b.close()
        assert len(a) == len(b) == len(c) == 3
        seen = 0
        for k, (x, y, z) in enumerate(zip(a, b, c)):
            token, pm, spec, frames, desc, jdesc, mdesc, label, idx = x
            n = label.shape[0]
            P = want_p[k]
            assert len(x) == 9 and n == (3 if k < 2 else 1)
            assert token.shape == (n, 1, 256) and token.dtype == torch.int64 and pm.shape == (n, 1, 256) and pm.dtype == torch.float32
            assert spec.shape == (n, 1024, 128) and spec.dtype == torch.float32
            assert desc.shape == (P, 12) and jdesc.shape == (P, 7) and mdesc.shape == (n, 4) and mdesc.dtype == torch.int64
            assert mdesc[:, :3].tolist() == mask[seen:seen + n].tolist() and mdesc[:, 3].tolist() == want_slots[k]
            assert label.tolist() == labels[seen:seen + n] and idx[:, 0].tolist() == list(range(seen, seen + n))
            ops.modal3_assemble_check(mdesc.clone(), P, OUT)
            ops.image_augment_check(desc.clone(), jdesc.clone(), frames.numel(), OUT, OUT)
            off = 0
            for j in range(n):
                i, m = seen + j, mask[seen + j]
                # rows of absent modalities are unspecified (never filled); rows of present ones hold the files, in every variant
                if m[0]:
                    fb = np.load(os.path.join(audio, names[i] + ".npy"))
                    assert all(np.array_equal(v[2][j].numpy(), fb) for v in (x, y, z))
                if m[2]:
                    tk, p_ = np.load(os.path.join(text, names[i] + "_token.npy")), np.load(os.path.join(text, names[i] + "_pm.npy"))
                    assert all(np.array_equal(v[0][j].numpy(), tk) and np.array_equal(v[1][j].numpy(), p_) for v in (x, y, z))
                if m[1]:
                    s = int(mdesc[j, 3])
                    d = os.path.join(visual, names[i])
                    want = decode_jpeg(os.path.join(d, pick_middle_frame(d)))
                    o, H, W = (int(v) for v in desc[s, :3])
                    assert o == off and (H, W) == want.shape[:2]                # packed back to back, present images only
                    assert np.array_equal(frames[o:o + H * W * 3].numpy().reshape(H, W, 3), want)
                    off += H * W * 3
                    assert torch.equal(desc[s, 1:], m3[3][i, 1:]) and torch.equal(jdesc[s], m3[4][i])
            assert frames.numel() == off
            for u, v, w in zip(x[3:], y[3:], z[3:]):                            # frames, descriptors, label, idx: bit-identical
                assert torch.equal(u, v) and torch.equal(u, w)
            seen += n
    # the mask is fixed; set_epoch reseeds the image draws only
    fb = Modal3Batcher(names, labels, 3, text, audio, frame_cache=cache, seed=4, pin=False, out_size=OUT, mask=mask)
    e0 = _clone(fb)
    fb.set_epoch(1)
    e1 = _clone(fb)
    assert all(torch.equal(p[6], q[6]) for p, q in zip(e0, e1))
    assert not torch.equal(e1[1][5], e0[1][5]) and not torch.equal(e1[1][4], e0[1][4])

    # nothing of an absent modality is opened: with those files gone, iteration still succeeds, from either source
    _delete_absent(mask, names, text, audio, visual)
    for i, m in enumerate(mask):
        if not m[1]:
            shutil.rmtree(os.path.join(cache, names[i]))
    for source in ({"visual_feature_path": visual}, {"frame_cache": cache}):
        got = _clone(Modal3Batcher(names, labels, 3, text, audio, threads=2, seed=4, pin=False, out_size=OUT, mask=mask, **source))
        for g, w in zip(got, e0):
            assert all(torch.equal(u, v) for u, v in zip(g[3:], w[3:]))
    # ... and a present file that is missing is an error, whichever modality it belongs to
    os.remove(os.path.join(audio, names[3] + ".npy"))                          # sample 3: audio + image
    with pytest.raises(MLAHipError, match="clip3.npy"):
        _clone(Modal3Batcher(names, labels, 3, text, audio, frame_cache=cache, pin=False, out_size=OUT, mask=mask))
    os.remove(os.path.join(text, names[2] + "_pm.npy"))                         # sample 2: text only
    with pytest.raises(MLAHipError, match="clip2_pm.npy"):
        _clone(Modal3Batcher(names[:3], labels[:3], 3, text, audio, frame_cache=cache, pin=False, out_size=OUT, mask=mask[:3]))
    shutil.rmtree(os.path.join(visual, names[1]))                               # sample 1: image only
    with pytest.raises(MLAHipError, match="clip1"):
        _clone(Modal3Batcher(names[:2], labels[:2], 3, text, audio, visual_feature_path=visual, pin=False, out_size=OUT, mask=mask[:2]))


def test_modal3_batcher_mask_arguments(tmp_path):
    names, labels = [f"clip{i}" for i in range(40)], [0] * 40
    kw = dict(frame_cache=str(tmp_path), pin=False)
    fb = Modal3Batcher(names, labels, 8, "t", "a", **kw)
    assert fb.mask.dtype == np.int64 and fb.mask.shape == (40, 3) and (fb.mask == 1).all()          # mask_percent = 0
    fb = Modal3Batcher(names, labels, 8, "t", "a", mask_percent=0.3, mask_seed=7, **kw)
    assert np.array_equal(fb.mask, random_mask(3, 40, 0.3, np.random.RandomState(7)))
    assert not np.array_equal(fb.mask, Modal3Batcher(names, labels, 8, "t", "a", mask_percent=0.3, mask_seed=1, **kw).mask)
    one = Modal3Batcher(names, labels, 8, "t", "a", mask_percent=0.8, **kw).mask
    assert (one.sum(axis=1) == 1).all()
    given = np.tile(np.array(ALL_ROWS), (6, 1))[:40]
    assert np.array_equal(Modal3Batcher(names, labels, 8, "t", "a", mask=given, mask_percent=0.5, **kw).mask, given)
    zero = given.copy()
    zero[5] = 0
    with pytest.raises(ValueError, match="sample 5 has no modality"):
        Modal3Batcher(names, labels, 8, "t", "a", mask=zero, **kw)
    with pytest.raises(ValueError, match="mask"):
        Modal3Batcher(names, labels, 8, "t", "a", mask=given[:39], **kw)
    with pytest.raises(ValueError, match="mask"):
        Modal3Batcher(names, labels, 8, "t", "a", mask=given * 2, **kw)
    with pytest.raises(ValueError):
        Modal3Batcher(names, labels, 8, "t", "a")
    with pytest.raises(MLAHipError, match="random_mask"):
        Modal3Batcher(names[:8], labels[:8], 8, "t", "a", mask_percent=0.3, **kw)                  # 10000 rounds of 8 x 3 draws
