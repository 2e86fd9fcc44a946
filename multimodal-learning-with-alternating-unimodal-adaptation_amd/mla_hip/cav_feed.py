"""CAVDataset batches (dataset/dataset.py:163-325, `--lorb large`) -> CAVClassifier inputs on the device.

The reference reads, per sample, one fbank .npy and the MIDDLE frame of the clip's directory, and transforms both on the CPU:

    image (dataset.py:251-256)   Resize(224, BICUBIC), CenterCrop(224), ToTensor(), Normalize(mean, std); train and eval alike
    fbank (dataset.py:281-321)   train and --cav_augnois: FrequencyMasking(48), TimeMasking(192);  always: (x + 5.081) / 4.4849;
                                 train and --cav_augnois: + rand(1024, 128) * np.random.rand() / 10, roll(randint(-1024, 1024), 0)

Here the host only decodes (or memcpys a frame `decode_middle_frames` decoded once), draws the few scalars of the augmentation
and packs descriptors; the work runs in two HIP kernels behind the batch's copies:

    csrc/frames.hip  mla_image_resample   crop -> Pillow-exact bicubic resize to the Resize(size) shape, of which only the
                                          CenterCrop window is computed -> LUT (ToTensor + Normalize); bit-identical to PIL
    csrc/fbank.hip   mla_fbank_augment    masks -> normalise -> Philox noise -> roll; bit-identical to torch's CPU result of the
                                          reference's expressions given the same uniforms

torchvision and torchaudio are restated, as frames.py restates RandomResizedCrop: Resize(int) / CenterCrop size arithmetic in
`resize_center_crop`, torchaudio.functional.mask_along_axis in `sample_fbank_aug`.  Every draw, and the Philox stream of the
noise, is a function of (seed, epoch, dataset index): batches do not depend on thread count, ring depth or rank.  (The
reference draws from per-worker global numpy / torch streams, so its own sequence is not reproducible; the distributions and
the order of the draws are what is matched.)

The same image transform at size 256 is the M3AE / Food-101 EVAL transform (dataset.py:413-420); the M3AE train transform
(timm create_transform with color jitter) is `m3ae_feed.M3AEBatcher`.  CAVDataset returns a 3-tuple without idx; CAVBatcher
yields idx like the other batchers.  The mixup branch of get_image (`filename2`) is never called and not reproduced.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError
from .data import FBANK_SHAPE
from .frames import (MEAN, STD, Batcher, ImagePart, Part, Placement, SampleKey, decode_frames, list_frames, sample_generator,
                     slot_buffer)
from .wav_feed import audio_fields, audio_part

NORM_MEAN, NORM_STD = -5.081, 4.4849           # dataset.py:259-260
FREQM, TIMEM = 48, 192                         # dataset.py:281
BILINEAR, BICUBIC = 0, 1                       # mla_image_resample's filter argument


def resize_center_crop(H: int, W: int, size: int) -> Tuple[int, int, int, int]:
    """torchvision Resize(size) + CenterCrop(size) on an H x W image: (full_h, full_w, win_top, win_left).  The short side
    becomes `size`, the long side int(size * long / short); the crop offsets use Python's round (halves go to even)."""
    if W <= H:
        ow, oh = size, int(size * H / W)
    else:
        oh, ow = size, int(size * W / H)
    return oh, ow, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


def image_descriptors(shapes: Sequence[Tuple[int, int]], boxes: Sequence[Tuple[int, int, int, int, int]],
                      windows: Sequence[Tuple[int, int, int, int]]) -> Tuple[np.ndarray, int]:
    """Pack frames back to back: int64 (N, 12) rows (byte offset, H, W, top, left, h, w, flip, full_h, full_w, win_top,
    win_left) and the total byte count."""
    desc = np.zeros((len(shapes), 12), dtype=np.int64)
    off = 0
    for n, ((H, W), box, win) in enumerate(zip(shapes, boxes, windows)):
        desc[n] = (off, H, W) + tuple(box) + tuple(win)
        off += H * W * 3
    return desc, off


def pick_middle_frame(visual_path: str) -> str:
    """File name of the frame CAVDataset reads (dataset.py:308-310): os.listdir order, NOT sorted, entry int(n / 2)."""
    allimages = list_frames(visual_path)
    return allimages[int(len(allimages) / 2)]


def decode_middle_frames(visual_feature_path: str, out_path: str, names: Sequence[str], threads: int = 16) -> int:
    """decode_frames for CAVBatcher(frame_cache=out_path): each sample's middle frame as <out_path>/<name>/0.npy."""
    return decode_frames(visual_feature_path, out_path, names, threads=threads, picker=lambda d: [pick_middle_frame(d)])


def _mask_along_axis(g: torch.Generator, mask_param: int, size: int) -> Tuple[int, int]:
    """torchaudio.functional.mask_along_axis's draws on `g`: (mask_start, mask_end - mask_start)."""
    value = torch.rand(1, generator=g) * mask_param
    min_value = torch.rand(1, generator=g) * (size - value)
    return int(min_value.long().item()), int(value.long().item())


def sample_fbank_aug(g: torch.Generator, T: int = FBANK_SHAPE[0], F: int = FBANK_SHAPE[1], freqm: int = FREQM,
                     timem: int = TIMEM) -> Tuple[int, int, int, int, float, int]:
    """(f0, fw, t0, tw, s, roll) of one sample in the reference's order: frequency mask, time mask (dataset.py:287-290), the
    noise scale s = np.random.rand() (a double in [0, 1)) and roll = np.random.randint(-T, T) (dataset.py:320-321)."""
    f0, fw = _mask_along_axis(g, freqm, F) if freqm != 0 else (0, 0)
    t0, tw = _mask_along_axis(g, timem, T) if timem != 0 else (0, 0)
    s = torch.rand(1, generator=g, dtype=torch.float64).item()
    roll = int(torch.randint(-T, T, (1,), generator=g).item())
    return f0, fw, t0, tw, s, roll


def fbank_stream_id(seed: int, epoch: int, index: int) -> int:
    """The Philox stream of a sample's noise: 63 bits from (seed, epoch, dataset index), independent of sample_generator's."""
    return int(np.random.SeedSequence([int(seed), int(epoch), int(index)]).generate_state(2, dtype=np.uint64)[1] >> np.uint64(1))


def fbank_descriptors(draws: Sequence[Optional[Tuple[int, int, int, int, float, int]]], stream_ids: Sequence[int]) -> np.ndarray:
    """int64 (B, 8) rows (flags, f0, fw, t0, tw, roll, scale_bits, stream_id); a draw of None gives flags = 0 (the sample is
    only normalised).  scale_bits is the bit pattern of fp32(s): torch casts the Python scalar to the tensor's dtype."""
    desc = np.zeros((len(draws), 8), dtype=np.int64)
    for b, (d, sid) in enumerate(zip(draws, stream_ids)):
        if d is not None:
            f0, fw, t0, tw, s, roll = d
            desc[b, :7] = (1, f0, fw, t0, tw, roll, int(np.float32(s).view(np.uint32)))
        desc[b, 7] = sid
    return desc


def middle_frame_path(visual: str, name: str, T: int = 1) -> List[str]:
    """Frame source of CAVDataset and Modal3Dataset for frames.ImagePart: the middle frame of the directory <visual>/<name>."""
    d = os.path.join(visual, name)
    return [os.path.join(d, pick_middle_frame(d))]


class ResizeCenterCrop:
    """Transform for frames.ImagePart: the whole frame through Resize(size, BICUBIC) + CenterCrop(size); no flip, no draws."""
    cols, kernel, filter = 12, "image_resample", BICUBIC

    def __init__(self, size: int):
        self.size = int(size)

    def place(self, shapes: Sequence[Tuple[int, int]], key: SampleKey) -> List[Placement]:
        return [Placement((0, 0, H, W, 0), resize_center_crop(H, W, self.size)) for (H, W) in shapes]

    @staticmethod
    def table(shapes, placed: Sequence[Placement]) -> Tuple[np.ndarray, int]:
        return image_descriptors(shapes, [p.crop for p in placed], [p.window for p in placed])


class FbankDraws(NamedTuple):
    masks_noise_roll: Optional[Tuple[int, int, int, int, float, int]]      # sample_fbank_aug's result; None: only normalised
    stream_id: int


class SpecAugPart(Part):
    """CAVDataset's spectrogram transform, listed after frames.fbank_part: a sample's SpecAug draws when `on` (train and
    --cav_augnois) and its noise stream as "fdesc" (B, 8); the device step replaces the raw "spec" the fbank part left in `out`
    by mla_fbank_augment's result (which is always normalised) in the slot's own buffer."""
    tensors = {"fdesc": (1, (8,), torch.int64)}

    def __init__(self, on: bool, norm_mean: float, norm_std: float, seed: int):
        self.on, self.norm_mean, self.norm_std, self.seed = bool(on), float(norm_mean), float(norm_std), int(seed)

    def load(self, name: str, key: SampleKey) -> FbankDraws:
        return FbankDraws(sample_fbank_aug(sample_generator(*key), *FBANK_SHAPE) if self.on else None, fbank_stream_id(*key))

    def pack(self, st: dict, recs: Sequence[FbankDraws], b: int, empty) -> dict:
        st["fdesc"][:b].numpy()[...] = fbank_descriptors([r.masks_noise_roll for r in recs], [r.stream_id for r in recs])
        return {"fdesc": st["fdesc"][:b]}

    def device(self, host: dict, dev: dict, scratch: dict, out: dict, B: int) -> None:
        raw = out["spec"]
        buf = slot_buffer(scratch, "spec", raw.shape[0], B, FBANK_SHAPE, torch.float32, raw.device)
        out["spec"] = ops.fbank_augment(raw, buf, dev["fdesc"], host["fdesc"], self.norm_mean, self.norm_std, self.seed)


class CAVBatcher(Batcher):
    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, audio_feature_path: Optional[str] = None,
                 visual_feature_path: Optional[str] = None, frame_cache: Optional[str] = None, train: bool = True,
                 augnois: bool = False, seed: int = 0, epoch: int = 0, threads: int = 8, ring: int = 4, pin: Optional[bool] = None,
                 drop_last: bool = False, out_size: int = 224, mean: Sequence[float] = MEAN, std: Sequence[float] = STD,
                 norm_mean: float = NORM_MEAN, norm_std: float = NORM_STD, audio_wav_path: Optional[str] = None):
        """CAVDataset batches from the fbank .npy files and either the JPEG frame directories (`visual_feature_path`) or a
        decode_middle_frames cache (`frame_cache`), on frames.Batcher's loop, staging ring, `copied()` fence and `device_step()` hook.
        Yields host tuples (spec_raw, frames uint8 (capacity,), image_desc int64 (B, 12), fbank_desc int64 (B, 8), label, idx);
        through a DeviceFeeder the device tuple is (spec (B, 1024, 128), image (B, 3, out, out), label, idx), the shapes
        CAVClassifier.forward takes.  The spectrogram is augmented only when `train and augnois` and always normalised; the
        image transform is the same in train and eval.  out_size=256 gives the M3AE / Food-101 eval transform.
        Audio: exactly one of `audio_feature_path` (fbank .npy files) and `audio_wav_path` (.wav files: wav_feed); with the latter
        the host tuple carries wav int16 (capacity,) and wdesc int64 (B, 4) where it carried spec_raw."""
        images = ImagePart(visual_feature_path, frame_cache, middle_frame_path, 1, ResizeCenterCrop(out_size), out_size, mean, std)
        if float(norm_std) == 0.0:
            raise ValueError("norm_std must not be 0")
        self.audio, self.audio_wav = audio_feature_path, audio_wav_path
        parts = [images, audio_part(audio_feature_path, audio_wav_path), SpecAugPart(train and augnois, norm_mean, norm_std, seed)]
        super().__init__(names, labels, batch_size, parts, audio_fields(("spec", "frames", "desc", "fdesc", "label", "idx"), audio_wav_path),
                         ("spec", "image", "label", "idx"), seed=seed, epoch=epoch, threads=threads, ring=ring, pin=pin,
                         drop_last=drop_last)
