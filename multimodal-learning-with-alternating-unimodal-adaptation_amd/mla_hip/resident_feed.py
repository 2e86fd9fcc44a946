"""The HBM-resident CREMA-D feed: the decoded dataset is uploaded once and a batch is three launches (csrc/resident.hip).

`FrameBatcher` + `DeviceFeeder` spend most of a fed step on the host: per sample they open files, copy 2 MB into pinned staging and
make a dozen torch.Generator draws, all of it contending for the GIL with the trainer's launch thread.  The card
holds the whole decoded training set many times over (6 698 clips: 10.4 GB of uint8 frames, 3.5 GB of fp32 fbanks), so here

    ResidentStore          uploads every frame (decode_frames layout and order), the frame table, the labels and the fbanks once;
    ResidentFrameBatcher   uploads an epoch's visiting order once per epoch and makes each batch with ops.resident_batch: the device
                           draws RandomResizedCrop(out) + RandomHorizontalFlip per frame, resamples straight out of the resident
                           buffer with FrameBatcher's kernel body and gathers the fbank rows.

Per batch the host does the launches and nothing else: no file, no copy, no draw, no thread pool, no synchronisation.

The draw is torchvision's algorithm (scale (0.08, 1), ratio (3/4, 4/3), ten tries, central-crop fallback, flip with p = 0.5) on
Philox4x32-10 in fp64, a function of (seed, epoch, dataset index, frame slot) alone; include/mla_hip.h (mla_resident_batch) defines it
word for word.  Its SEQUENCE differs from FrameBatcher's for the same seed (that one draws from a torch.Generator per sample); the
algorithm and the distribution are the same, as they are between FrameBatcher and the reference's unreproducible worker streams.
Unlike the disk batchers this one shuffles (`shuffle=True`, main.py:814), with clip_feed.epoch_permutation.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError
from .clip_feed import epoch_permutation
from .data import FBANK_SHAPE, load_fbank
from .frames import MAX_THREADS, MEAN, OUT_SIZE, PICK_NUM, STD, _CachedFrame, _cache_path, decode_jpeg, frame_paths, make_lut

STAGING_BYTES = 64 << 20
FBANK_BYTES = FBANK_SHAPE[0] * FBANK_SHAPE[1] * 4


def _jpeg_shape(path: str) -> Tuple[int, int]:
    from PIL import Image
    try:
        with Image.open(path) as im:                             # the header only: nothing is decoded
            return im.size[1], im.size[0]
    except Exception as e:
        raise MLAHipError(f"{path}: cannot read ({e})") from e


def frame_table(names: Sequence[str], frame_cache: Optional[str] = None, visual_feature_path: Optional[str] = None,
                pick_num: int = PICK_NUM) -> Tuple[torch.Tensor, int, List[List[str]]]:
    """The store's frame table without reading a pixel: host int64 (N * T, 3) rows (byte offset, H, W), frames packed back to back
    in decode_frames order (sample after sample, time slot after time slot), the total byte count, and each sample's T files."""
    if (visual_feature_path is None) == (frame_cache is None):
        raise ValueError("give exactly one of visual_feature_path (JPEG frames) and frame_cache (decode_frames output)")
    T = int(pick_num)
    table = np.zeros((len(names) * T, 3), dtype=np.int64)
    files, off = [], 0
    for i, name in enumerate(names):
        paths = [_cache_path(frame_cache, name, t) for t in range(T)] if frame_cache is not None else \
            frame_paths(visual_feature_path, name, T)
        for t, p in enumerate(paths):
            if frame_cache is not None:
                f = _CachedFrame(p)
                H, W = f.shape[:2]
                f.close()
            else:
                H, W = _jpeg_shape(p)
            table[i * T + t] = (off, H, W)
            off += H * W * 3
        files.append(paths)
    return torch.from_numpy(table), off, files


class _Uploader:
    """Host -> device through two pinned staging buffers of `nbytes`: `reserve(n)` hands out n bytes of staging (numpy uint8),
    `send(dst)` copies what was reserved since the last send into the device bytes `dst`; a buffer is refilled only after its
    copy has completed."""

    def __init__(self, nbytes: int, device):
        self.device = device
        self.bufs = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.events: List[Optional[torch.cuda.Event]] = [None, None]
        self.k, self.used, self.cap = 0, 0, nbytes

    def room(self, n: int) -> bool:
        return self.used + n <= self.cap

    def reserve(self, n: int) -> np.ndarray:
        if self.used == 0 and self.events[self.k] is not None:
            self.events[self.k].synchronize()
        a = self.bufs[self.k].numpy()[self.used:self.used + n]
        self.used += n
        return a

    def send(self, dst: torch.Tensor) -> None:
        if self.used:
            dst.copy_(self.bufs[self.k][:self.used], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.events[self.k] = ev
            self.k, self.used = 1 - self.k, 0

    def finish(self) -> None:
        for ev in self.events:
            if ev is not None:
                ev.synchronize()


class ResidentStore:
    """The uploaded dataset: `frames` (device uint8, every frame in decode_frames layout and order), `table` (device int64
    (N * T, 3): byte offset, H, W) and `table_host`, `labels` (device int64 (N,)), `spec` (device fp32 (N, 1024, 128), or None
    when no audio source is given).  It is an object of its own so that the feeds of other datasets can share it.

    Frames come from exactly one of `frame_cache` (the decode_frames output) and `visual_feature_path` (the JPEG directories,
    decoded once here with frame_paths + decode_jpeg in at most 16 threads); audio from at most one of `audio_feature_path` (fbank
    .npy files) and `audio_wav_path` (.wav files, whose fbank ops.wav_fbank computes once here in chunks: the bits of
    wav_feed.extract_fbank).  The bytes are totalled from the file headers before anything is allocated, and a dataset above
    `max_bytes` (default: 80 % of the free device memory) is refused.  The upload goes through two pinned staging buffers of
    `staging_bytes`.  `nbytes` is what is resident."""

    def __init__(self, names: Sequence[str], labels: Sequence[int], *, frame_cache: Optional[str] = None,
                 visual_feature_path: Optional[str] = None, audio_feature_path: Optional[str] = None,
                 audio_wav_path: Optional[str] = None, pick_num: int = PICK_NUM, max_bytes: Optional[int] = None, device="cuda",
                 threads: int = MAX_THREADS, staging_bytes: int = STAGING_BYTES):
        if len(names) != len(labels):
            raise ValueError("names and labels differ in length")
        if len(names) == 0:
            raise MLAHipError("ResidentStore: no samples")
        if audio_feature_path is not None and audio_wav_path is not None:
            raise ValueError("give at most one of audio_feature_path (fbank .npy files) and audio_wav_path (.wav files)")
        self.names, self.N, self.T = list(names), len(names), int(pick_num)
        self.table_host, self.frames_bytes, files = frame_table(self.names, frame_cache, visual_feature_path, self.T)
        has_audio = audio_feature_path is not None or audio_wav_path is not None
        spec_bytes = self.N * FBANK_BYTES if has_audio else 0
        self.nbytes = self.frames_bytes + spec_bytes + self.table_host.numel() * 8 + self.N * 8
        if max_bytes is None:
            max_bytes = int(0.8 * torch.cuda.mem_get_info(torch.device(device))[0])
        if self.nbytes > max_bytes:
            raise MLAHipError(f"ResidentStore: {self.N} samples need {self.nbytes} bytes on the device ({self.frames_bytes} of frames, "
                              f"{spec_bytes} of spectrograms), more than max_bytes = {int(max_bytes)}")
        self.device = torch.device(device)
        self._plans: dict = {}
        self.labels = torch.as_tensor(np.asarray(labels, dtype=np.int64)).to(self.device)
        self.table = self.table_host.to(self.device)
        self.frames = torch.empty(self.frames_bytes, dtype=torch.uint8, device=self.device)
        biggest = int((self.table_host[:, 1] * self.table_host[:, 2] * 3).max())
        up = _Uploader(max(int(staging_bytes), biggest), self.device)
        self._upload_frames(up, files, frame_cache is not None, max(1, min(int(threads), MAX_THREADS)))
        self.spec = None
        if audio_feature_path is not None:
            self.spec = torch.empty((self.N,) + FBANK_SHAPE, dtype=torch.float32, device=self.device)
            self._upload_fbanks(up, audio_feature_path)
        up.finish()
        if audio_wav_path is not None:
            self.spec = torch.empty((self.N,) + FBANK_SHAPE, dtype=torch.float32, device=self.device)
            self._compute_fbanks(audio_wav_path, max(1, min(int(threads), MAX_THREADS)))

    def _upload_frames(self, up: _Uploader, files: List[List[str]], cached: bool, threads: int) -> None:
        rows = self.table_host.numpy()
        flat = [p for paths in files for p in paths]
        with ThreadPoolExecutor(threads) as pool:
            n0 = 0
            while n0 < len(flat):                                # a run of frames that fits the staging buffer
                n1, size = n0, 0
                while n1 < len(flat) and up.room(size + int(rows[n1, 1] * rows[n1, 2] * 3)):
                    size += int(rows[n1, 1] * rows[n1, 2] * 3)
                    n1 += 1
                stage, base = up.reserve(size), int(rows[n0, 0])

                def one(n):
                    o, H, W = (int(v) for v in rows[n])
                    dst = stage[o - base:o - base + H * W * 3]
                    if cached:
                        f = _CachedFrame(flat[n])
                        if f.shape[:2] != (H, W):
                            f.close()
                            raise MLAHipError(f"{flat[n]}: the frame changed size while the store was built")
                        f.copy_to(dst)
                    else:
                        a = decode_jpeg(flat[n])
                        if a.shape != (H, W, 3):
                            raise MLAHipError(f"{flat[n]}: decoded to {a.shape}, its header said ({H}, {W}, 3)")
                        np.copyto(dst.reshape(H, W, 3), a)
                list(pool.map(one, range(n0, n1)))
                up.send(self.frames[base:base + size])
                n0 = n1

    def _upload_fbanks(self, up: _Uploader, path: str) -> None:
        flat = self.spec.view(-1).view(torch.uint8)
        start = pos = 0                                          # the device bytes [start, pos) are staged and not yet sent
        for name in self.names:
            row = np.ascontiguousarray(load_fbank(path, name)).view(np.uint8).reshape(-1)
            o = 0
            while o < FBANK_BYTES:                               # a row may span staging buffers
                if not up.room(1):
                    up.send(flat[start:pos])
                    start = pos
                n = min(FBANK_BYTES - o, up.cap - up.used)
                np.copyto(up.reserve(n), row[o:o + n])
                o, pos = o + n, pos + n
        up.send(flat[start:pos])

    def _compute_fbanks(self, path: str, threads: int, chunk: int = 64) -> None:
        from .wav_feed import WavPart, clip_descriptors, device_tables
        part, tables = WavPart(path), device_tables(self.device)
        with ThreadPoolExecutor(threads) as pool:
            for i0 in range(0, self.N, chunk):
                recs = list(pool.map(lambda i: part.load(self.names[i], None), range(i0, min(i0 + chunk, self.N))))
                desc, total = clip_descriptors([r.samples for r in recs])
                wav = np.concatenate([r.samples for r in recs])
                assert wav.shape[0] == total
                desc_host = torch.from_numpy(desc)
                ops.wav_fbank(torch.from_numpy(wav).to(self.device), desc_host.to(self.device), desc_host, tables,
                              self.spec[i0:i0 + len(recs)])
        torch.cuda.current_stream().synchronize()                # the host arrays above are pageable: their copies have been made

    def plan(self, out_h: int, out_w: int, train: bool) -> ops.ResidentPlan:
        """The resample plan of this dataset for one output size, computed once (ops.resident_plan)."""
        key = (int(out_h), int(out_w), bool(train))
        if key not in self._plans:
            self._plans[key] = ops.resident_plan(self.table_host, self.T, self.frames_bytes, out_h, out_w, train)
        return self._plans[key]


class ResidentFrameBatcher:
    """AVDataset batches (dataset.py:111-161) out of a ResidentStore.  Iterating yields the device tuple
    (spec (b, 1024, 128), image (b, 3, T, out, out), label (b,), idx (b, 1)) that DeviceFeeder(FrameBatcher) yields, so MLATrainer,
    JointTrainer and QMFTrainer take it unchanged.  `set_epoch(e)` makes clip_feed.epoch_permutation(N, shuffle, seed, e), checks it
    and uploads it once; iterating before it uses epoch 0.  `train=False`: whole frames, no flip.

    Give `store=`, or the source arguments of ResidentStore (exactly one frame source and exactly one audio source, as FrameBatcher
    requires), from which a store is built.

    Slot contract: every batch is enqueued on the CURRENT stream into one of `depth` output slots, in turn.  A yielded batch stays
    untouched until `depth` further batches have been yielded.  Stream order is the only fence: the trainers' calling stream waits
    for every forward before train_step returns (feed.py), so by the time the launches that refill a slot run on that stream,
    nothing reads it any more.  There is no copy stream, no event and no thread pool.  A consumer that reads a batch on another
    stream must make that stream wait for the current one, and the current one for its reads, itself.
    `last_desc` is the device descriptor table (b * T, 8) of the batch yielded last (tests, debugging)."""

    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, *, store: Optional[ResidentStore] = None,
                 frame_cache: Optional[str] = None, visual_feature_path: Optional[str] = None,
                 audio_feature_path: Optional[str] = None, audio_wav_path: Optional[str] = None, train: bool = True,
                 shuffle: bool = False, seed: int = 0, drop_last: bool = False, out_size: int = OUT_SIZE, pick_num: int = PICK_NUM,
                 mean: Sequence[float] = MEAN, std: Sequence[float] = STD, depth: int = 2, max_bytes: Optional[int] = None,
                 device="cuda"):
        if len(names) != len(labels):
            raise ValueError("names and labels differ in length")
        if batch_size <= 0:
            raise MLAHipError(f"ResidentFrameBatcher: batch_size must be positive, got {batch_size}")
        if not 0 <= int(seed) < 1 << 32:
            raise MLAHipError(f"ResidentFrameBatcher: seed {seed} must lie in [0, 2^32)")
        sources = (frame_cache, visual_feature_path, audio_feature_path, audio_wav_path)
        if store is None:
            if (audio_feature_path is None) == (audio_wav_path is None):
                raise ValueError("give exactly one of audio_feature_path (fbank .npy files) and audio_wav_path (.wav files)")
            store = ResidentStore(names, labels, frame_cache=frame_cache, visual_feature_path=visual_feature_path,
                                  audio_feature_path=audio_feature_path, audio_wav_path=audio_wav_path, pick_num=pick_num,
                                  max_bytes=max_bytes, device=device)
        elif any(s is not None for s in sources):
            raise ValueError("give either store= or the source arguments, not both")
        if store.spec is None:
            raise MLAHipError("ResidentFrameBatcher: the store holds no spectrograms (build it with an audio source)")
        if store.names != list(names) or store.T != int(pick_num):
            raise MLAHipError("ResidentFrameBatcher: the store was built from other names or another pick_num")
        self.store, self.names, self.B, self.T = store, list(names), int(batch_size), store.T
        self.train, self.shuffle, self.seed, self.drop_last = bool(train), bool(shuffle), int(seed), bool(drop_last)
        self.out_size, self.depth, self.device = int(out_size), max(1, int(depth)), store.device
        self.N = store.N
        self.labels = store.labels if [int(x) for x in labels] == store.labels.tolist() else \
            torch.as_tensor(np.asarray(labels, dtype=np.int64)).to(self.device)
        self.plan = store.plan(self.out_size, self.out_size, self.train)
        self.lut = make_lut(mean, std).to(self.device)
        self.epoch = 0
        self._order: Optional[torch.Tensor] = None
        self._slots: List[Optional[tuple]] = [None] * self.depth
        self._next = 0
        self.last_desc: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return self.N // self.B if self.drop_last else (self.N + self.B - 1) // self.B

    def set_epoch(self, epoch: int) -> None:
        if not 0 <= int(epoch) < 1 << 32:
            raise MLAHipError(f"ResidentFrameBatcher: epoch {epoch} must lie in [0, 2^32)")
        perm = epoch_permutation(self.N, self.shuffle, self.seed, epoch)
        ops.gather_index_check(perm, self.N)                         # the range check, where the index is produced
        self.epoch = int(epoch)
        self._order = perm.to(self.device)                           # uploaded once per epoch

    def _slot(self) -> tuple:
        k = self._next
        self._next = (k + 1) % self.depth
        if self._slots[k] is None:
            B, T, S, dev = self.B, self.T, self.out_size, self.device
            self._slots[k] = (torch.empty((B,) + FBANK_SHAPE, dtype=torch.float32, device=dev),
                              torch.empty((B, 3, T, S, S), dtype=torch.float32, device=dev),
                              torch.empty(B, dtype=torch.int64, device=dev), torch.empty((B, 1), dtype=torch.int64, device=dev),
                              torch.empty((B * T, 8), dtype=torch.int64, device=dev))
        return self._slots[k]

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, ...]]:
        if self._order is None:
            self.set_epoch(self.epoch)
        order, epoch, st = self._order, self.epoch, self.store
        for k in range(len(self)):
            pos = k * self.B
            b = min(self.B, self.N - pos)
            spec, image, label, idx, desc = self._slot()
            spec, image, label, idx, desc = spec[:b], image[:b], label[:b], idx[:b], desc[:b * self.T]
            ops.resident_batch(st.frames, st.table, st.spec, self.labels, order, self.T, pos, b, self.seed, epoch, self.train, self.plan,
                               self.lut, desc, image, spec, label, idx)
            self.last_desc = desc
            yield spec, image, label, idx
