"""CLIPFeatureBatcher: the batch feed of CLIPClassifier from device-resident feature tables.

The reference's CLIPDataset (dataset/dataset.py:806-877) reads `<text>/<name>.npy` and `<visual>/<name>.npy` -- one (1, D) fp32
array per sample and modality -- in every __getitem__, and the loader collates and copies a batch to the device per step.  The
whole Food-101 feature set is about 280 MB, so here both tables and the labels are read once, uploaded once and stay on the
device; a batch is ONE `mla_gather_rows2` launch over the epoch's index vector (uploaded once per epoch): no per-batch host copy,
no host synchronisation in the loop.

Host half (`load_feature_tables`, `epoch_permutation`) needs no GPU.
"""
from __future__ import annotations

import os
from typing import Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MLAHipError


def _load_feature(path: str) -> np.ndarray:
    """One stored feature as fp32 (D,): fp32 or fp16 (widened exactly) of shape (1, D) or (D,); anything else is refused."""
    try:
        a = np.load(path, allow_pickle=False)
    except Exception as e:                                   # missing file, truncated file, pickled payload, ...
        raise MLAHipError(f"{path}: cannot read ({e})") from e
    if a.dtype not in (np.dtype(np.float32), np.dtype(np.float16)) or not ((a.ndim == 2 and a.shape[0] == 1) or a.ndim == 1) \
            or a.shape[-1] == 0:
        raise MLAHipError(f"{path}: expected float32 (1, D) or (D,), found {a.dtype.name}{tuple(a.shape)}")
    return a.reshape(-1).astype(np.float32)


def load_feature_tables(names: Sequence[str], text_feature_path: str, visual_feature_path: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(token (N, D), visual (N, D)) host fp32 tables, row i = sample names[i] (dataset/dataset.py:864-872); the same D everywhere."""
    if len(names) == 0:
        raise MLAHipError("CLIPFeatureBatcher: no samples")
    tabs = []
    D = None
    for root in (text_feature_path, visual_feature_path):
        rows = []
        for name in names:
            path = os.path.join(root, name + ".npy")
            a = _load_feature(path)
            if D is None:
                D = a.shape[0]
            if a.shape[0] != D:
                raise MLAHipError(f"{path}: feature width {a.shape[0]} differs from the first file's {D}")
            rows.append(a)
        tabs.append(torch.from_numpy(np.stack(rows)))
    return tabs[0], tabs[1]


def epoch_permutation(n: int, shuffle: bool, seed: int, epoch: int) -> torch.Tensor:
    """The epoch's visiting order (host int64): the identity, or with `shuffle` a function of (seed, epoch) alone."""
    if not shuffle:
        return torch.arange(n, dtype=torch.int64)
    gen = torch.Generator(device="cpu")
    gen.manual_seed((int(seed) * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randperm(n, generator=gen, dtype=torch.int64)


class CLIPFeatureBatcher:
    """Iterating yields (token (B, 1, D), image (B, 1, D), label (B,), idx (B, 1)) device tensors, as the reference's loader
    does for --clip (main.py:139-148, 428-429); `set_epoch(e)` draws the order (the identity without `shuffle`)."""

    def __init__(self, names: Sequence[str], labels: Sequence[int], batch_size: int, text_feature_path: str,
                 visual_feature_path: str, shuffle: bool = False, seed: int = 0, drop_last: bool = False, device="cuda"):
        if len(names) != len(labels):
            raise MLAHipError(f"CLIPFeatureBatcher: {len(names)} names but {len(labels)} labels")
        if batch_size <= 0:
            raise MLAHipError(f"CLIPFeatureBatcher: batch_size must be positive, got {batch_size}")
        self.names, self.B = list(names), int(batch_size)
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        self.device = torch.device(device)
        tok, vis = load_feature_tables(self.names, text_feature_path, visual_feature_path)
        self.N, self.D = tok.shape
        self.token = tok.to(self.device)                             # uploaded once
        self.visual = vis.to(self.device)
        self.labels = torch.as_tensor(np.asarray(labels, dtype=np.int64)).to(self.device)
        self.epoch = 0
        self._order = None

    def __len__(self) -> int:
        return self.N // self.B if self.drop_last else (self.N + self.B - 1) // self.B

    def set_epoch(self, epoch: int) -> None:
        perm = epoch_permutation(self.N, self.shuffle, self.seed, epoch)
        ops.gather_index_check(perm, self.N)                         # the range check, where the index is produced
        self.epoch = int(epoch)
        self._order = perm.to(self.device)                           # uploaded once per epoch

    def __iter__(self):
        if self._order is None:
            self.set_epoch(self.epoch)
        order = self._order
        f32 = dict(device=self.device, dtype=torch.float32)
        for k in range(len(self)):
            idx = order[k * self.B:(k + 1) * self.B]                 # a view: no copy, no sync
            b = idx.numel()
            token, image = torch.empty((b, 1, self.D), **f32), torch.empty((b, 1, self.D), **f32)
            label = torch.empty(b, device=self.device, dtype=torch.int64)
            oidx = torch.empty((b, 1), device=self.device, dtype=torch.int64)
            ops.gather_rows2(self.token, self.visual, self.labels, idx, token.view(b, self.D), image.view(b, self.D), label, oidx)
            yield token, image, label, oidx
