"""CREMA-D video frames -> augmented batches on the device (dataset/dataset.py:120-161).

The reference decodes, crops, resizes, flips and normalises every frame on the CPU in 32 DataLoader workers (main.py:785):
about 4 ms of CPU per frame, some 35 cores at the training step's rate.  Here the host only decodes (or memcpys frames that
`decode_frames` decoded once) and packs uint8 frames plus one descriptor per frame; crop, bilinear resize, flip, ToTensor
and Normalize run in one HIP kernel (csrc/frames.hip) that is bit-identical to PIL + torchvision:

    train (dataset.py:129-135)   RandomResizedCrop(224), RandomHorizontalFlip(), ToTensor(), Normalize(mean, std)
    eval  (dataset.py:136-140)   Resize((224, 224)), ToTensor(), Normalize(mean, std)

Frame choice (dataset.py:121-143): `os.listdir` order, NOT sorted (the reference does not sort either), seg = int(n / 3),
frames seg * i for i = 0, 1, 2.  A directory with fewer than 3 files gives seg = 0 and so frame 0 three times; that is the
reference's behaviour and is kept.

Random draws: torchvision's RandomResizedCrop.get_params and RandomHorizontalFlip restated on a torch.Generator per sample,
seeded from (seed, epoch, dataset index), frame after frame in time order.  Batches therefore do not depend on thread count,
ring depth or rank.  (The reference's 32 workers draw from per-worker streams, so its own sequence is not reproducible; the
distribution and the algorithm are what is matched.)

`FrameBatcher` yields host tuples (spec, frames, desc, label, idx) from a ring of pinned staging buffers and implements
DeviceFeeder's `copied()` and `device_step()` hooks: fed through a DeviceFeeder, the kernel runs on the feeder's copy stream
behind the batch's copies and the feeder yields the reference's tuple (spec, image (B, 3, 3, 224, 224) fp32, label, idx).

CAVDataset's feed (bicubic Resize + CenterCrop of the middle frame, fbank SpecAug) and the M3AE / Food-101 eval transform
(the same at size 256) are in `cav_feed` (CAVBatcher subclasses FrameBatcher: same staging ring, fences and hooks); the M3AE /
Food-101 timm TRAIN transform (dataset.py:401-412: bicubic random crop, flip, color jitter) is in `m3ae_feed` (M3AEBatcher);
Modal3Dataset's three-modality feed with its missing-modality masks (dataset.py:596-803) is in `modal3_feed` (Modal3Batcher).
Out of scope: QMF's masking.
"""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError
from .data import FBANK_SHAPE, load_fbank

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # dataset.py:134, 139
PICK_NUM, OUT_SIZE = 3, 224                                     # dataset.py:142, 130, 137
SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)              # RandomResizedCrop defaults
MAX_THREADS = 16
_LOG_RATIO = torch.log(torch.tensor(RATIO))     # torchvision: torch.log(torch.tensor(ratio)), fp32


def make_lut(mean: Sequence[float] = MEAN, std: Sequence[float] = STD) -> torch.Tensor:
    """fp32 (3, 256): lut[c][u] = ToTensor + Normalize of the byte u in channel c, with the torch CPU ops torchvision runs
    (img.float().div(255), then tensor.sub_(mean).div_(std)) -- the kernel's normalisation is a lookup, exact by construction."""
    x = torch.arange(256, dtype=torch.uint8).float().div(255).expand(3, 256).contiguous()
    m = torch.as_tensor(mean, dtype=torch.float32)
    s = torch.as_tensor(std, dtype=torch.float32)
    return x.sub_(m[:, None]).div_(s[:, None])


def pick_frames(visual_path: str, pick_num: int = PICK_NUM) -> List[str]:
    """File names of the frames the reference reads from one sample's directory (dataset.py:121-143), in time order."""
    try:
        allimages = os.listdir(visual_path)
    except OSError as e:
        raise MLAHipError(f"{visual_path}: cannot list frames ({e})") from e
    if not allimages:
        raise MLAHipError(f"{visual_path}: no frames")
    seg = int(len(allimages) / pick_num)
    return [allimages[int(seg * i)] for i in range(pick_num)]


def sample_generator(seed: int, epoch: int, index: int) -> torch.Generator:
    """The per-sample generator of the draws: a function of (seed, epoch, dataset index) only."""
    s = int(np.random.SeedSequence([int(seed), int(epoch), int(index)]).generate_state(1, dtype=np.uint64)[0])
    return torch.Generator().manual_seed(s)


def sample_crop(height: int, width: int, g: torch.Generator, scale=SCALE, ratio=RATIO) -> Tuple[int, int, int, int]:
    """torchvision RandomResizedCrop.get_params on `g`: (top, left, h, w)."""
    area = height * width
    log_ratio = _LOG_RATIO if tuple(ratio) == RATIO else torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0].item(), log_ratio[1].item(), generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
            return int(i), int(j), h, w
    in_ratio = float(width) / float(height)          # fallback: central crop
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def sample_flip(g: torch.Generator, p: float = 0.5) -> bool:
    """torchvision RandomHorizontalFlip: torch.rand(1) < p."""
    return bool(torch.rand(1, generator=g).item() < p)


def sample_augment(shapes: Sequence[Tuple[int, int]], g: Optional[torch.Generator], train: bool) -> List[Tuple[int, int, int, int, int]]:
    """(top, left, h, w, flip) per frame of one sample.  train: crop then flip draws, frame after frame (the reference
    applies its transform to each frame in turn).  eval: the whole frame, no flip, no draws (Resize((224, 224)))."""
    out = []
    for (H, W) in shapes:
        if train:
            box = sample_crop(H, W, g)
            out.append(box + (int(sample_flip(g)),))
        else:
            out.append((0, 0, H, W, 0))
    return out


def frame_descriptors(shapes: Sequence[Tuple[int, int]], boxes: Sequence[Tuple[int, int, int, int, int]]) -> Tuple[np.ndarray, int]:
    """Pack frames back to back: int64 (N, 8) rows (byte offset, H, W, top, left, h, w, flip) and the total byte count."""
    desc = np.zeros((len(shapes), 8), dtype=np.int64)
    off = 0
    for n, ((H, W), box) in enumerate(zip(shapes, boxes)):
        desc[n] = (off, H, W) + tuple(box)
        off += H * W * 3
    return desc, off


def decode_jpeg(path: str) -> np.ndarray:
    """uint8 (H, W, 3): np.asarray(Image.open(path).convert('RGB')) (dataset.py:146)."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))
    except Exception as e:
        raise MLAHipError(f"{path}: cannot decode ({e})") from e


def _cache_path(frame_cache: str, name: str, t: int) -> str:
    return os.path.join(frame_cache, name, f"{t}.npy")


def load_cached_frame(frame_cache: str, name: str, t: int) -> np.ndarray:
    """Time slot t of a sample from the decode_frames cache, memory-mapped; uint8 (H, W, 3) checked like data._load."""
    path = _cache_path(frame_cache, name, t)
    try:
        a = np.load(path, mmap_mode="r", allow_pickle=False)
    except Exception as e:
        raise MLAHipError(f"{path}: cannot read ({e})") from e
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
        raise MLAHipError(f"{path}: expected uint8 (H, W, 3), found {a.dtype.name}{tuple(a.shape)}")
    return a


class _CachedFrame:
    """A decode_frames file whose header has been read and checked: `copy_to` reads the pixels straight into the staging
    buffer (one copy out of the page cache, GIL released; no mmap, whose page faults serialise the loader threads)."""

    def __init__(self, path: str):
        self.path = path
        try:
            self.f = open(path, "rb")
            version = np.lib.format.read_magic(self.f)
            read = {(1, 0): np.lib.format.read_array_header_1_0, (2, 0): np.lib.format.read_array_header_2_0}.get(version)
            if read is None:
                raise ValueError(f"npy format version {version}")
            shape, fortran, dtype = read(self.f)
        except Exception as e:
            self.close()
            raise MLAHipError(f"{path}: cannot read ({e})") from e
        if dtype != np.uint8 or len(shape) != 3 or shape[2] != 3 or shape[0] == 0 or shape[1] == 0 or fortran:
            self.close()
            raise MLAHipError(f"{path}: expected uint8 (H, W, 3), found {dtype.name}{tuple(shape)}")
        self.shape, self.size = tuple(shape), int(np.prod(shape))

    def close(self):
        if getattr(self, "f", None) is not None:
            self.f.close()
            self.f = None

    def copy_to(self, dst: np.ndarray) -> None:
        try:
            n = self.f.readinto(memoryview(dst.reshape(-1)))
        finally:
            self.close()
        if n != self.size:
            raise MLAHipError(f"{self.path}: truncated ({n} of {self.size} pixel bytes)")


def decode_frames(visual_feature_path: str, out_path: str, names: Sequence[str], pick_num: int = PICK_NUM,
                  threads: int = MAX_THREADS, picker=None) -> int:
    """Decode each sample's picked JPEGs once with PIL into <out_path>/<name>/<t>.npy (uint8 HWC, t = time slot 0..2, in the
    order pick_frames returns them).  FrameBatcher(frame_cache=out_path) then gives batches bit-identical to the JPEG source
    with a memcpy per frame instead of a decode.  Returns the number of files written.
    `picker(directory) -> file names` replaces pick_frames(directory, pick_num): cav_feed.decode_middle_frames caches the one
    frame CAVDataset reads as time slot 0."""
    def one(name):
        d = os.path.join(visual_feature_path, name)
        frames = pick_frames(d, pick_num) if picker is None else list(picker(d))
        os.makedirs(os.path.join(out_path, name), exist_ok=True)
        for t, f in enumerate(frames):
            np.save(_cache_path(out_path, name, t), decode_jpeg(os.path.join(visual_feature_path, name, f)))
        return len(frames)
    with ThreadPoolExecutor(max(1, min(int(threads), MAX_THREADS))) as pool:
        return sum(pool.map(one, names))


class FrameBatcher:
    DESC_COLS = 8                 # columns of a frame descriptor row (cav_feed.CAVBatcher: 12)

    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, audio_feature_path: str,
                 visual_feature_path: Optional[str] = None, frame_cache: Optional[str] = None, train: bool = True,
                 seed: int = 0, epoch: int = 0, threads: int = 8, ring: int = 4, pin: Optional[bool] = None,
                 drop_last: bool = False, out_size: int = OUT_SIZE, pick_num: int = PICK_NUM,
                 mean: Sequence[float] = MEAN, std: Sequence[float] = STD):
        """AVDataset batches (dataset.py:111-161) from the fbank .npy files and either the JPEG frame directories
        (`visual_feature_path`, decoded with PIL in a pool of `threads` <= 16 threads) or a decode_frames cache
        (`frame_cache`).  Yields host tuples (spec, frames uint8 (capacity,), desc int64 (B*T, 8), label, idx); through a
        DeviceFeeder the device tuple is (spec, image (B, 3, T, out, out) fp32, label, idx).  `set_epoch` reseeds the draws.
        Threads: the cache source is fastest with threads=1 (a memcpy per frame; more threads contend for the GIL), the
        JPEG source gains up to about 8."""
        if (visual_feature_path is None) == (frame_cache is None):
            raise ValueError("give exactly one of visual_feature_path (JPEG frames) and frame_cache (decode_frames output)")
        if len(names) != len(labels):
            raise ValueError("names and labels differ in length")
        self.names, self.labels, self.B = list(names), [int(x) for x in labels], int(batch_size)
        self.audio, self.visual, self.cache = audio_feature_path, visual_feature_path, frame_cache
        self.train, self.seed, self.epoch = bool(train), int(seed), int(epoch)
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.T, self.size, self.drop_last = int(pick_num), int(out_size), drop_last
        self.lut = make_lut(mean, std)
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        # staging ring + fences: the same protocol as data.NpyBatcher (a tuple is refilled only after the copies out of it ran)
        self.ring = max(2, ring)
        self._stage: List[Optional[dict]] = [None] * self.ring
        self._fence: List[Optional[object]] = [None] * self.ring
        self._unfenced: List[int] = []
        self._pool: Optional[ThreadPoolExecutor] = None

    def __len__(self) -> int:
        n = len(self.names)
        return n // self.B if self.drop_last else (n + self.B - 1) // self.B

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def close(self) -> None:
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None

    def sample_frames(self, i: int) -> List[np.ndarray]:
        """The T decoded uint8 (H, W, 3) frames of dataset index i, from the JPEGs or the cache."""
        name = self.names[i]
        if self.cache is not None:
            return [load_cached_frame(self.cache, name, t) for t in range(self.T)]
        d = os.path.join(self.visual, name)
        return [decode_jpeg(os.path.join(d, f)) for f in pick_frames(d, self.T)]

    def sample_boxes(self, i: int, shapes: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int, int, int]]:
        """(top, left, h, w, flip) per frame of dataset index i for the current epoch."""
        g = sample_generator(self.seed, self.epoch, i) if self.train else None
        return sample_augment(shapes, g, self.train)

    def _load(self, i: int):
        if self.cache is not None:
            frames = []
            try:
                for t in range(self.T):
                    frames.append(_CachedFrame(_cache_path(self.cache, self.names[i], t)))
            except MLAHipError:
                for f in frames:
                    f.close()
                raise
        else:
            frames = self.sample_frames(i)
        shapes = [f.shape[:2] for f in frames]
        return self._load_side(i), frames, self.sample_boxes(i, shapes)

    # what is loaded beside the frames: the fbank here, the token pair in m3ae_feed.M3AEBatcher
    def _load_side(self, i: int):
        return load_fbank(self.audio, self.names[i])

    def _side_staging(self, mk) -> dict:
        return {"spec": mk((self.B,) + FBANK_SHAPE, torch.float32)}

    def _fill_side(self, st: dict, j: int, side) -> None:
        np.copyto(st["spec"][j].numpy(), side)

    def _descriptors(self, shapes, boxes) -> Tuple[np.ndarray, int]:
        return frame_descriptors(shapes, boxes)

    def _extra_staging(self, mk) -> dict:
        """Further pinned staging tensors of a subclass's host tuple."""
        return {}

    def _fill_extra(self, st: dict, ids: Sequence[int], loaded: Sequence[tuple]) -> None:
        """Fill what _extra_staging added, from the batch's dataset indices and _load results."""

    def _host_tuple(self, st: dict, b: int) -> tuple:
        return st["spec"][:b], st["frames"], st["desc"][:b * self.T], st["label"][:b], st["idx"][:b]

    def _staging(self, k: int, nbytes: int) -> dict:
        st = self._stage[k]
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=self.pin)
        if st is None:
            st = {"desc": mk((self.B * self.T, self.DESC_COLS), torch.int64),
                  "label": mk((self.B,), torch.int64), "idx": mk((self.B, 1), torch.int64), "frames": None}
            st.update(self._side_staging(mk))
            st.update(self._extra_staging(mk))
            self._stage[k] = st
        if st["frames"] is None or st["frames"].numel() < nbytes:      # grows with the largest batch seen, in MiB steps
            cap = max(nbytes, 1, (st["frames"].numel() * 5 // 4) if st["frames"] is not None else 0)
            st["frames"] = mk(((cap + (1 << 20) - 1) >> 20) << 20, torch.uint8)
        return st

    def copied(self, event) -> None:
        """DeviceFeeder hook (see data.NpyBatcher.copied)."""
        if self._unfenced:
            self._fence[self._unfenced.pop(0)] = event

    def device_step(self, host: Sequence[torch.Tensor], dev: Sequence[torch.Tensor], scratch: dict) -> tuple:
        """DeviceFeeder hook, run on its copy stream behind the copies of `dev` (= `host` on the device): augment the frames
        into the slot's fp32 image buffer and return the reference's tuple (spec, image, label, idx)."""
        spec, frames, desc, label, idx = dev
        b = label.shape[0]
        img = scratch.get("image")
        if img is None or img.shape[0] < b:
            img = scratch["image"] = torch.empty((max(b, self.B), 3, self.T, self.size, self.size), dtype=torch.float32,
                                                 device=spec.device)
        if "lut" not in scratch:
            scratch["lut"] = self.lut.to(spec.device)
        out = ops.frames_resample(frames, desc, host[2], scratch["lut"], img[:b], self.T)
        return spec, out, label, idx

    def __iter__(self) -> Iterator[tuple]:
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.threads)
        k = 0
        self._unfenced = []
        batches = [list(range(b0, min(b0 + self.B, len(self.names)))) for b0 in range(0, len(self.names), self.B)]
        if self.drop_last and batches and len(batches[-1]) < self.B:
            batches.pop()
        submit = lambda ids: [self._pool.submit(self._load, i) for i in ids]       # decode (or open) + draws, one task per sample
        pending = submit(batches[0]) if batches else []
        for bi, ids in enumerate(batches):
            b = len(ids)
            loaded = [f.result() for f in pending]
            first = np.cumsum([0] + [len(l[1]) for l in loaded])        # a sample's first descriptor row: j * T, unless a subclass's
            shapes = [f.shape[:2] for l in loaded for f in l[1]]          # _load leaves frames out (modal3_feed: a masked-out image)
            boxes = [box for l in loaded for box in l[2]]
            desc, nbytes = self._descriptors(shapes, boxes)
            if self._fence[k] is not None:
                self._fence[k].synchronize()
                self._fence[k] = None
            if k in self._unfenced:
                self._unfenced.remove(k)
            st = self._staging(k, nbytes)
            buf = st["frames"].numpy()

            def fill(j):
                side, frames = loaded[j][:2]
                self._fill_side(st, j, side)
                for t, f in enumerate(frames):
                    o = int(desc[first[j] + t, 0])
                    if isinstance(f, _CachedFrame):
                        f.copy_to(buf[o:o + f.size])
                    else:
                        np.copyto(buf[o:o + f.size].reshape(f.shape), f)
            list(self._pool.map(fill, range(b)))
            st["desc"][:len(desc)].numpy()[...] = desc
            st["label"][:b] = torch.tensor([self.labels[i] for i in ids], dtype=torch.int64)
            st["idx"][:b, 0] = torch.tensor(ids, dtype=torch.int64)
            self._fill_extra(st, ids, loaded)
            self._unfenced.append(k)
            pending = submit(batches[bi + 1]) if bi + 1 < len(batches) else []     # the next batch loads while this one is consumed
            yield self._host_tuple(st, b)
            k = (k + 1) % self.ring
