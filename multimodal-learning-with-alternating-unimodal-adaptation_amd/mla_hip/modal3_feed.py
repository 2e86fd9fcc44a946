"""Modal3Dataset batches (dataset/dataset.py:596-803; IEMOCAP, `--modal3`) -> Modal3Classifier inputs on the device, with the
reference's missing-modality masks.

The reference reads, per sample, `<text>/<name>_token.npy`, `<text>/<name>_pm.npy`, the MIDDLE file of `os.listdir(<visual>/<name>)`
(unsorted, entry int(n / 2): cav_feed.pick_middle_frame) and `<audio>/<name>.npy`:

    image (dataset.py:697-716)   train: timm create_transform(256, is_training=True, color_jitter=True, "bicubic", re_prob=0);
                                 eval: Resize(256, BICUBIC), CenterCrop(256), ToTensor(), Normalize -- M3AEBatcher's transforms
    fbank (dataset.py:788-790)   raw: norm_mean / norm_std are set and never applied, and there is no SpecAug
    mask  (dataset.py:794-801)   m = maskmatrix[idx]; spectrogram * m[0], image * m[1], tokenizer * m[2], padding_mask * m[2]

`maskmatrix = random_mask(3, n, args.mask_percent)` is drawn once, when the dataset is built, from numpy's global legacy stream
(main.py defines no --mask_percent, so the reference's own modal3 run stops with an AttributeError; here it is a constructor
parameter).  `random_mask` below makes the same draws in the same order on a RandomState: with np.random.seed(s) there and
RandomState(s) here the matrices are equal (tests/golden/modal3_mask_small.npz).

A masked-out modality costs nothing on the host: no np.load of the fbank or of the token pair, no decode, no frame in the packed
buffer and no descriptor row.  The image kernels (csrc/frames.hip) run over the P images the batch does have, into a compact
(P, 3, S, S) buffer; csrc/modal3.hip's mla_modal3_assemble then places them, writes zeros for the others and zeroes the staged rows
of absent spectrograms, tokens and padding masks (which hold whatever the pinned ring held before) in one launch behind the
batch's copies.  The zeros are +0.0 where the reference's x * 0 gives -0.0 for negative x: equal values, torch.equal holds.
On the device the encoders run on those zeros unless the step is told which rows are there: Modal3Batcher.present(step) gives the
batch's mask rows for MLATrainer.train_step(..., present=) / Evaluator.update(..., present=) (mla_hip.rows).

Every image draw is a function of (seed, epoch, dataset index), as in M3AEBatcher: a sample's crop, flip and jitter do not depend
on whether its neighbours are masked.  The mask is fixed for the batcher's life, as in the reference; set_epoch reseeds the image
draws only.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError
from .cav_feed import middle_frame_path
from .data import batch_ids
from .frames import MEAN, RATIO, SCALE, STD, Batcher, Part, SampleKey, slot_buffer, token_part
from .wav_feed import audio_fields, audio_part
from .m3ae_feed import OUT_SIZE, timm_image_part

AUDIO, IMAGE, TEXT = 0, 1, 2                   # columns of the mask matrix (dataset.py:798-801)
MASK_TOLERANCE = 0.005                         # dataset.py:619


def random_mask(view_num: int, n: int, missing_rate: float, rng: np.random.RandomState, max_iter: int = 10000) -> np.ndarray:
    """The reference's random_mask (dataset.py:596-640) on `rng`: int64 (n, view_num) of 0/1 with at least one 1 per row and
    a share of ones within 0.005 of 1 - missing_rate.  OneHotEncoder(categories=[arange(view_num)]).fit_transform(r).toarray()
    is eye(view_num)[r[:, 0]].  Three regimes: 1 - missing_rate <= 1 / view_num keeps exactly one modality per sample (float64
    in the reference, int64 here); missing_rate == 0 is all ones; otherwise the rejection loop.  The reference's loop never ends
    when no matrix can meet the tolerance (n = 8 at rate 0.3: 24 entries, and 17/24 and 16/24 are both further than 0.005 from
    0.7); after `max_iter` rounds this raises MLAHipError.  A round whose overlap correction divides by zero (where the
    reference stops with an OverflowError) counts as a failed round."""
    one_rate = 1 - missing_rate
    eye = np.eye(view_num, dtype=np.int64)
    if one_rate <= (1 / view_num):
        return eye[rng.randint(0, view_num, size=(n, 1))[:, 0]]
    if one_rate == 1:
        return rng.randint(1, 2, size=(n, view_num)).astype(np.int64)
    for _ in range(int(max_iter)):
        view_preserve = eye[rng.randint(0, view_num, size=(n, 1))[:, 0]]
        one_num = view_num * n * one_rate - n
        ratio = one_num / (view_num * n)
        matrix_iter = (rng.randint(0, 100, size=(n, view_num)) < int(ratio * 100)).astype(np.int64)
        a = int(np.sum(((matrix_iter + view_preserve) > 1).astype(np.int64)))
        if 1 - a / one_num == 0:
            continue
        one_num_iter = one_num / (1 - a / one_num)
        ratio = one_num_iter / (view_num * n)
        matrix_iter = (rng.randint(0, 100, size=(n, view_num)) < int(ratio * 100)).astype(np.int64)
        matrix = ((matrix_iter + view_preserve) > 0).astype(np.int64)
        ratio = np.sum(matrix) / (view_num * n)
        if abs(one_rate - ratio) < MASK_TOLERANCE:
            return matrix
    raise MLAHipError(f"random_mask: no {n} x {view_num} mask within {MASK_TOLERANCE} of a share of ones of {one_rate:g} (missing rate "
                      f"{missing_rate:g}) in {int(max_iter)} rounds")


def mask_descriptors(rows: np.ndarray) -> np.ndarray:
    """int64 (B, 4) rows (audio present, image present, text present, image slot) from a batch's mask rows (B, 3): the images
    that are present take the slots 0, 1, ... in batch order, the others -1."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    desc = np.empty((rows.shape[0], 4), dtype=np.int64)
    desc[:, :3] = rows
    desc[:, 3] = np.where(rows[:, IMAGE] != 0, np.cumsum(rows[:, IMAGE] != 0) - 1, -1)
    return desc


class MaskPart(Part):
    """Modal3Batcher's own part, last in its list: the batch's mask rows as "mdesc" (B, 4), and the one extra device step,
    mla_modal3_assemble, over what the parts before it left in `out`: the compact images become "image" (B, 3, size, size)
    and the rows of absent spectrograms, tokens and padding masks are zeroed."""
    tensors = {"mdesc": (1, (4,), torch.int64)}

    def __init__(self, mask: np.ndarray, size: int):
        self.mask, self.size = mask, int(size)

    def load(self, name: str, key: SampleKey) -> np.ndarray:
        return self.mask[key.index]

    def pack(self, st: dict, recs: Sequence[np.ndarray], b: int, empty) -> dict:
        st["mdesc"][:b].numpy()[...] = mask_descriptors(np.stack(recs))
        return {"mdesc": st["mdesc"][:b]}

    def device(self, host: dict, dev: dict, scratch: dict, out: dict, B: int) -> None:
        mdesc, S = dev["mdesc"], self.size
        image = slot_buffer(scratch, "assembled", mdesc.shape[0], B, (3, S, S), torch.float32, mdesc.device)
        out["image"] = ops.modal3_assemble(out["image"], out["spec"], out["token"], out["pm"], mdesc, host["mdesc"], image)


class Modal3Batcher(Batcher):
    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, text_feature_path: str, audio_feature_path: Optional[str] = None,
                 visual_feature_path: Optional[str] = None, frame_cache: Optional[str] = None, train: bool = True,
                 mask_percent: float = 0.0, mask_seed: int = 0, mask=None, seed: int = 0, epoch: int = 0, threads: int = 8,
                 ring: int = 4, out_size: int = OUT_SIZE, scale: Sequence[float] = SCALE, ratio: Sequence[float] = RATIO,
                 color_jitter=1.0, mean: Sequence[float] = MEAN, std: Sequence[float] = STD, drop_last: bool = False,
                 pin: Optional[bool] = None, audio_wav_path: Optional[str] = None):
        """Modal3Dataset batches from the token / padding-mask and fbank .npy files and either the JPEG frame directories
        (`visual_feature_path`) or a decode_middle_frames cache (`frame_cache`), on frames.Batcher's loop, staging ring, `copied()`
        fence and `device_step()` hook.  `self.mask` int64 (n, 3), columns (audio, image, text), is random_mask(3, n, mask_percent,
        RandomState(mask_seed)) unless `mask` gives it (0/1 entries, no all-zero row: the reference keeps one modality per sample).
        Yields host tuples (token, padding_mask, spec, frames uint8 (capacity,), image_desc int64 (P, 12), jitter_desc int64
        (P, 7), mask_desc int64 (B, 4), label, idx), P = the batch's images that are present; rows of token, padding_mask and
        spec whose modality is absent are NOT filled.  Through a DeviceFeeder the device tuple is (token (B, 1, 256) int64,
        padding_mask (B, 1, 256) fp32, image (B, 3, out, out) fp32, spec (B, 1024, 128) fp32, label, idx): Modal3Dataset.__getitem__'s
        tuple, MLATrainer.train_step's argument order, with absent modalities zero.  Image transform and its arguments: M3AEBatcher.
        Audio: exactly one of `audio_feature_path` (fbank .npy files) and `audio_wav_path` (.wav files: wav_feed); with the latter
        the host tuple carries wav int16 (capacity,) and wdesc int64 (B, 4) where it carried spec, an absent spectrogram is a
        wdesc row with n_samples = 0, and no .wav is opened for it."""
        n = len(names)
        if mask is None:
            mask = random_mask(3, n, float(mask_percent), np.random.RandomState(int(mask_seed)))
        mask = np.asarray(mask)
        if mask.shape != (n, 3) or not np.isin(mask, (0, 1)).all():
            raise ValueError(f"mask: expected ({n}, 3) entries 0 / 1 in columns (audio, image, text), got shape {mask.shape}")
        if n and (mask.sum(axis=1) == 0).any():
            raise ValueError(f"mask: sample {int(np.argmin(mask.sum(axis=1)))} has no modality left (the reference keeps at least one)")
        self.mask = mask.astype(np.int64)
        self.text, self.audio, self.audio_wav = text_feature_path, audio_feature_path, audio_wav_path
        have = self.mask != 0
        parts = [timm_image_part(visual_feature_path, frame_cache, middle_frame_path, train, out_size, scale, ratio, color_jitter,
                                 mean, std, present=have[:, IMAGE]),
                 token_part(text_feature_path, present=have[:, TEXT]),
                 audio_part(audio_feature_path, audio_wav_path, present=have[:, AUDIO]),
                 MaskPart(self.mask, out_size)]
        super().__init__(names, labels, batch_size, parts,
                         audio_fields(("token", "pm", "spec", "frames", "desc", "jdesc", "mdesc", "label", "idx"), audio_wav_path),
                         ("token", "pm", "image", "spec", "label", "idx"), seed=seed, epoch=epoch, threads=threads, ring=ring,
                         pin=pin, drop_last=drop_last)

    def present(self, step: int) -> torch.Tensor:
        """Host bool (b, 3), columns (audio, image, text): the mask rows of the batch the iterator yields at position `step` (batches
        are in dataset order), as Modal3Classifier / MLATrainer.train_step / Evaluator.update take them under `present=`."""
        return torch.from_numpy(self.mask[batch_ids(len(self.names), self.B, self.drop_last)[step]] != 0)
