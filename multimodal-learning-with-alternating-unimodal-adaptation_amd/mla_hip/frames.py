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

This module also holds what the batchers of every dataset are put together from: `Batcher`, the shared loop (batching, thread
pool, prefetch, data.StagingRing, `copied()`, `device_step()`), and the three parts a batch is made of, `fbank_part`, `token_part`
and `ImagePart` (interface: `Part`).  A batcher is a Batcher subclass whose constructor lists its parts and the order of its
tuples; none overrides the loop.  The sibling modules add frame sources and transforms for ImagePart, and their batchers:
    cav_feed      CAVBatcher: the middle frame through bicubic Resize + CenterCrop (also the M3AE / Food-101 eval transform, at
                  size 256), fbank normalise + SpecAug (SpecAugPart, listed after fbank_part)
    m3ae_feed     M3AEBatcher: <name>.jpg through the timm TRAIN transform (dataset.py:401-412: bicubic random crop, flip,
                  color jitter), token pair
    modal3_feed   Modal3Batcher: Modal3Dataset's three modalities with its missing-modality masks (dataset.py:596-803)
    wav_feed      WavPart: <name>.wav in place of the fbank <name>.npy (`audio_wav_path=` of FrameBatcher, CAVBatcher and
                  Modal3Batcher), the Kaldi fbank computed on the device
Out of scope: QMF's masking.
"""
from __future__ import annotations

import math
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError
from .data import FBANK_SHAPE, TOKEN_SHAPE, StagingRing, batch_ids, load_fbank, load_token

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


def list_frames(visual_path: str) -> List[str]:
    """os.listdir of one sample's frame directory, in its order (NOT sorted); an unreadable or empty directory is an error."""
    try:
        allimages = os.listdir(visual_path)
    except OSError as e:
        raise MLAHipError(f"{visual_path}: cannot list frames ({e})") from e
    if not allimages:
        raise MLAHipError(f"{visual_path}: no frames")
    return allimages


def pick_frames(visual_path: str, pick_num: int = PICK_NUM) -> List[str]:
    """File names of the frames the reference reads from one sample's directory (dataset.py:121-143), in time order."""
    allimages = list_frames(visual_path)
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
    """Time slot t of a sample from the decode_frames cache: uint8 (H, W, 3), checked and read as the batchers read it."""
    f = _CachedFrame(_cache_path(frame_cache, name, t))
    a = np.empty(f.shape, dtype=np.uint8)
    f.copy_to(a)
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


# ---- the records that parts load per sample ------------------------------------------------------------------------------------
class SampleKey(NamedTuple):
    """What every random draw of a sample is a function of: sample_generator(*key)."""
    seed: int
    epoch: int
    index: int


class Placement(NamedTuple):
    """Where one frame goes in its output image: a transform's draws, one field per descriptor group."""
    crop: Tuple[int, int, int, int, int]             # top, left, h, w, flip
    window: Tuple[int, ...] = ()                     # full_h, full_w, win_top, win_left (12-column descriptors only)
    jitter: Optional[tuple] = None                   # a m3ae_feed.sample_jitter result


class Fbank(NamedTuple):
    spec: np.ndarray


class Tokens(NamedTuple):
    token: np.ndarray
    pm: np.ndarray


class Images(NamedTuple):
    frames: list                                     # decoded uint8 (H, W, 3) arrays, or _CachedFrame (read in `fill`)
    placed: List[Placement]                          # one per frame
    offsets: List[int]                               # byte offset per frame in the packed buffer; ImagePart.pack sets it


def slot_buffer(scratch: dict, key: str, n: int, B: int, shape: Tuple[int, ...], dtype, device) -> torch.Tensor:
    """n rows of scratch[key], a device tensor (max(n, B), *shape) of a DeviceFeeder slot that is allocated when first needed."""
    t = scratch.get(key)
    if t is None or t.shape[0] < n:
        t = scratch[key] = torch.empty((max(n, B),) + tuple(shape), dtype=dtype, device=device)
    return t[:n]


class Part:
    """One modality of a batch; a batcher is Batcher's loop plus a list of these.  A part names
        tensors                                its staging per ring slot: field -> (rows per sample, row shape, dtype); Batcher
                                               allocates B times as many rows
        load(name, key)                        what it reads and draws for one sample, a named record; runs inside the pool
        pack(st, recs, b, empty)               once per batch, with every sample's record: writes the tables and returns the host
                                               tensors it yields, by field (here: b rows of each of `tensors`)
        fill(st, j, rec)                       per sample inside the pool: copies the record into row j of the staging
        device(host, dev, scratch, out, B)     its share of device_step: adds to `out`, by field, and may work on what the
                                               parts before it put there
    `present` (bool per dataset index; None = all) tells a part which samples have it: for the others neither `load` nor `fill`
    is called (nothing is opened, their record is None and their staging rows keep whatever they held)."""
    tensors: dict = {}
    present = None

    def pack(self, st: dict, recs: Sequence, b: int, empty) -> dict:
        return {k: st[k][:b] for k in self.tensors}

    def fill(self, st: dict, j: int, rec) -> None:
        pass


class NpyPart(Part):
    """Rows read from one sample's .npy files, handed on as they are: `read(name)` returns a record with one array per field."""

    def __init__(self, read, tensors: dict, present=None):
        self.read, self.tensors, self.present = read, tensors, present

    def load(self, name: str, key: SampleKey):
        return self.read(name)

    def fill(self, st: dict, j: int, rec) -> None:
        for k in self.tensors:
            np.copyto(st[k][j].numpy(), getattr(rec, k))

    def device(self, host: dict, dev: dict, scratch: dict, out: dict, B: int) -> None:
        out.update((k, dev[k]) for k in self.tensors)


def fbank_part(path: str, present=None) -> NpyPart:
    """<path>/<name>.npy -> "spec" fp32 (B, 1024, 128), raw (cav_feed.SpecAugPart after it normalises and augments)."""
    return NpyPart(lambda name: Fbank(load_fbank(path, name)), {"spec": (1, FBANK_SHAPE, torch.float32)}, present)


def token_part(path: str, present=None) -> NpyPart:
    """<path>/<name>_token.npy and <name>_pm.npy -> "token" int64 and "pm" fp32, (B, 1, 256) each."""
    return NpyPart(lambda name: Tokens(*load_token(path, name)),
                   {"token": (1, TOKEN_SHAPE, torch.int64), "pm": (1, TOKEN_SHAPE, torch.float32)}, present)


def frame_paths(visual: str, name: str, T: int) -> List[str]:
    """Frame source of AVDataset: the T picked frames of the directory <visual>/<name>."""
    d = os.path.join(visual, name)
    return [os.path.join(d, f) for f in pick_frames(d, T)]


class RandomCropFlip:
    """AVDataset's transform: RandomResizedCrop + flip when `train`, else the whole frame; bilinear, mla_frames_resample."""
    cols, kernel = 8, "frames_resample"

    def __init__(self, train: bool):
        self.train = train

    def place(self, shapes: Sequence[Tuple[int, int]], key: SampleKey) -> List[Placement]:
        return [Placement(crop) for crop in sample_augment(shapes, sample_generator(*key) if self.train else None, self.train)]

    @staticmethod
    def table(shapes, placed: Sequence[Placement]) -> Tuple[np.ndarray, int]:
        return frame_descriptors(shapes, [p.crop for p in placed])


class ImagePart(Part):
    """Packed uint8 frames: "frames" (capacity,), one descriptor row per frame in "desc" and, with `jitter_table`, one jitter
    row per image in "jdesc"; the device step turns them into "image", fp32 (P, 3, T, size, size) over the P samples that have
    frames (None when P = 0), without the T axis unless `keep_time`.
    Frame source: the decode_frames-layout `cache`, time slots 0 .. T - 1, or the JPEGs that `paths(visual, name, T)` names
    (frame_paths, cav_feed.middle_frame_path, m3ae_feed.image_path).
    Transform: `place(shapes, key)` draws a sample's Placements, `table(shapes, placed)` packs a batch's descriptor rows of
    `cols` columns, and `kernel` names the op that runs them (RandomCropFlip, cav_feed.ResizeCenterCrop, m3ae_feed.TimmTrain)."""

    def __init__(self, visual: Optional[str], cache: Optional[str], paths, T: int, transform, size: int, mean, std,
                 keep_time: bool = False, jitter_table=None, present=None):
        if (visual is None) == (cache is None):
            raise ValueError("give exactly one of visual_feature_path (JPEG frames) and frame_cache (decode_frames output)")
        self.visual, self.cache, self.paths, self.T, self.transform, self.size = visual, cache, paths, int(T), transform, int(size)
        self.lut, self.keep_time, self.jitter_table, self.present = make_lut(mean, std), keep_time, jitter_table, present
        self.tensors = {"desc": (self.T, (transform.cols,), torch.int64)}
        if jitter_table:
            self.tensors["jdesc"] = (1, jitter_table([]).shape[1:], torch.int64)           # the table of no image has its width

    def decoded(self, name: str) -> List[np.ndarray]:
        """The sample's T decoded uint8 (H, W, 3) frames, from the JPEGs or the cache."""
        if self.cache is not None:
            return [load_cached_frame(self.cache, name, t) for t in range(self.T)]
        return [decode_jpeg(p) for p in self.paths(self.visual, name, self.T)]

    def load(self, name: str, key: SampleKey) -> Images:
        if self.cache is None:
            frames = self.decoded(name)
        else:
            frames = []
            try:
                for t in range(self.T):
                    frames.append(_CachedFrame(_cache_path(self.cache, name, t)))
            except MLAHipError:
                for f in frames:
                    f.close()
                raise
        return Images(frames, self.transform.place([f.shape[:2] for f in frames], key), [])

    def pack(self, st: dict, recs: Sequence[Optional[Images]], b: int, empty) -> dict:
        have = [r for r in recs if r is not None]
        placed = [p for r in have for p in r.placed]
        desc, nbytes = self.transform.table([f.shape[:2] for r in have for f in r.frames], placed)
        buf = st.get("frames")
        if buf is None or buf.numel() < nbytes:                        # grows with the largest batch seen, in MiB steps
            cap = max(nbytes, 1, (buf.numel() * 5 // 4) if buf is not None else 0)
            buf = st["frames"] = empty(((cap + (1 << 20) - 1) >> 20) << 20, torch.uint8)
        st["desc"][:len(desc)].numpy()[...] = desc
        host = {"frames": buf, "desc": st["desc"][:len(desc)]}
        if self.jitter_table:
            st["jdesc"][:len(placed)].numpy()[...] = self.jitter_table([p.jitter for p in placed])
            host["jdesc"] = st["jdesc"][:len(placed)]
        offsets = iter(desc[:, 0].tolist())
        for r in have:
            r.offsets[:] = [next(offsets) for _ in r.frames]
        return host

    def fill(self, st: dict, j: int, rec: Images) -> None:
        buf = st["frames"].numpy()
        for o, f in zip(rec.offsets, rec.frames):
            if isinstance(f, _CachedFrame):
                f.copy_to(buf[o:o + f.size])
            else:
                np.copyto(buf[o:o + f.size].reshape(f.shape), f)

    def device(self, host: dict, dev: dict, scratch: dict, out: dict, B: int) -> None:
        desc, S, kernel = dev["desc"], self.size, self.transform.kernel
        n = desc.shape[0] // self.T
        img = slot_buffer(scratch, "image", n, B, (3, self.T, S, S), torch.float32, desc.device)
        if "lut" not in scratch:
            scratch["lut"] = self.lut.to(desc.device)
        if n == 0:
            img = None
        elif kernel == "frames_resample":
            ops.frames_resample(dev["frames"], desc, host["desc"], scratch["lut"], img, self.T)
        elif kernel == "image_augment":
            ops.image_augment(dev["frames"], desc, host["desc"], dev["jdesc"], host["jdesc"], scratch["lut"], img,
                              slot_buffer(scratch, "staging", n, B, (S * S * 3,), torch.uint8, desc.device),
                              slot_buffer(scratch, "partials", n, B, (S,), torch.int64, desc.device))
        else:
            ops.image_resample(dev["frames"], desc, host["desc"], scratch["lut"], img, self.T, self.transform.filter)
        out["image"] = img if self.keep_time or n == 0 else img.view(n, 3, S, S)


class Batcher:
    """The loop every batcher of the family shares: batches of `batch_size` dataset indices (`drop_last`), one pool task per
    sample that loads every part's record, the next batch loading while the current one is consumed, a StagingRing of slots
    (one dict of staging tensors each) fenced through `copied()`, label and idx, and DeviceFeeder's `device_step()` hook.
    `parts` is the list of modality parts, `host_fields` the order of the yielded host tuple (the parts' fields, "label",
    "idx"), `device_fields` the order of the tuple device_step returns (what the parts put into `out`, "label", "idx")."""
    tensors = {"label": (1, (), torch.int64), "idx": (1, (1,), torch.int64)}

    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, parts: Sequence[Part], host_fields: Sequence[str],
                 device_fields: Sequence[str], seed: int = 0, epoch: int = 0, threads: int = 8, ring: int = 4,
                 pin: Optional[bool] = None, drop_last: bool = False):
        if len(names) != len(labels):
            raise ValueError("names and labels differ in length")
        self.names, self.labels, self.B = list(names), [int(x) for x in labels], int(batch_size)
        self.parts, self.host_fields, self.device_fields = list(parts), tuple(host_fields), tuple(device_fields)
        self.seed, self.epoch, self.drop_last = int(seed), int(epoch), drop_last
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self._ring = StagingRing(ring, pin)
        self._pool: Optional[ThreadPoolExecutor] = None

    def __len__(self) -> int:
        return len(batch_ids(len(self.names), self.B, self.drop_last))

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def close(self) -> None:
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None

    def copied(self, event) -> None:
        """DeviceFeeder hook (see data.StagingRing.copied)."""
        self._ring.copied(event)

    def device_step(self, host: Sequence[torch.Tensor], dev: Sequence[torch.Tensor], scratch: dict) -> tuple:
        """DeviceFeeder hook, run on its copy stream behind the copies of `dev` (= `host` on the device): every part's device
        work into the slot's buffers; returns the tensors named by `device_fields`."""
        host, dev = dict(zip(self.host_fields, host)), dict(zip(self.host_fields, dev))
        out = {"label": dev["label"], "idx": dev["idx"]}
        for part in self.parts:
            part.device(host, dev, scratch, out, self.B)
        return tuple(out[f] for f in self.device_fields)

    def _load(self, i: int) -> list:
        key = SampleKey(self.seed, self.epoch, i)
        return [part.load(self.names[i], key) if part.present is None or part.present[i] else None for part in self.parts]

    def __iter__(self) -> Iterator[tuple]:
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.threads)
        self._ring.restart()
        batches = batch_ids(len(self.names), self.B, self.drop_last)
        submit = lambda ids: [self._pool.submit(self._load, i) for i in ids]       # decode (or open) + draws, one task per sample
        pending = submit(batches[0]) if batches else []
        for bi, ids in enumerate(batches):
            b = len(ids)
            loaded = [f.result() for f in pending]                                 # per sample, one record per part
            k = self._ring.acquire()
            st = self._ring.slots[k]
            if st is None:
                st = self._ring.slots[k] = {f: self._ring.empty((self.B * rows,) + tuple(shape), dtype)
                                            for owner in [self] + self.parts for f, (rows, shape, dtype) in owner.tensors.items()}
            named = {"label": st["label"][:b], "idx": st["idx"][:b]}
            for part, recs in zip(self.parts, zip(*loaded)):
                named.update(part.pack(st, recs, b, self._ring.empty))

            def fill(j):
                for part, rec in zip(self.parts, loaded[j]):
                    if rec is not None:
                        part.fill(st, j, rec)
            list(self._pool.map(fill, range(b)))
            named["label"][:] = torch.tensor([self.labels[i] for i in ids], dtype=torch.int64)
            named["idx"][:, 0] = torch.tensor(list(ids), dtype=torch.int64)
            self._ring.yielded(k)
            pending = submit(batches[bi + 1]) if bi + 1 < len(batches) else []     # the next batch loads while this one is consumed
            yield tuple(named[f] for f in self.host_fields)


class FrameBatcher(Batcher):
    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, audio_feature_path: Optional[str] = None,
                 visual_feature_path: Optional[str] = None, frame_cache: Optional[str] = None, train: bool = True,
                 seed: int = 0, epoch: int = 0, threads: int = 8, ring: int = 4, pin: Optional[bool] = None,
                 drop_last: bool = False, out_size: int = OUT_SIZE, pick_num: int = PICK_NUM,
                 mean: Sequence[float] = MEAN, std: Sequence[float] = STD, audio_wav_path: Optional[str] = None):
        """AVDataset batches (dataset.py:111-161) from the fbank .npy files and either the JPEG frame directories
        (`visual_feature_path`, decoded with PIL in a pool of `threads` <= 16 threads) or a decode_frames cache
        (`frame_cache`).  Yields host tuples (spec, frames uint8 (capacity,), desc int64 (B*T, 8), label, idx); through a
        DeviceFeeder the device tuple is (spec, image (B, 3, T, out, out) fp32, label, idx).  `set_epoch` reseeds the draws.
        Threads: the cache source is fastest with threads=1 (a memcpy per frame; more threads contend for the GIL), the
        JPEG source gains up to about 8.
        Audio: exactly one of `audio_feature_path` (fbank .npy files) and `audio_wav_path` (16 kHz mono PCM16 .wav files, whose
        fbank mla_wav_fbank computes on the device: wav_feed); with the latter the host tuple carries wav int16 (capacity,) and
        wdesc int64 (B, 4) where it carried spec, and the device tuple is the same."""
        from .wav_feed import audio_fields, audio_part           # wav_feed builds on this module
        self.audio, self.audio_wav = audio_feature_path, audio_wav_path
        self.images = ImagePart(visual_feature_path, frame_cache, frame_paths, pick_num, RandomCropFlip(bool(train)), out_size,
                                mean, std, keep_time=True)
        super().__init__(names, labels, batch_size, [self.images, audio_part(audio_feature_path, audio_wav_path)],
                         audio_fields(("spec", "frames", "desc", "label", "idx"), audio_wav_path), ("spec", "image", "label", "idx"),
                         seed=seed, epoch=epoch, threads=threads, ring=ring, pin=pin, drop_last=drop_last)

    def sample_frames(self, i: int) -> List[np.ndarray]:
        """The T decoded uint8 (H, W, 3) frames of dataset index i, from the JPEGs or the cache."""
        return self.images.decoded(self.names[i])

    def sample_boxes(self, i: int, shapes: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int, int, int]]:
        """(top, left, h, w, flip) per frame of dataset index i for the current epoch."""
        return [p.crop for p in self.images.transform.place(shapes, SampleKey(self.seed, self.epoch, i))]
