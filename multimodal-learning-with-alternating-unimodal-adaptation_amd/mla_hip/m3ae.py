"""Transformer modality encoders on the HIP kernels: M3AE text / image (reference: models/m3ae.py:48-179,
300-370; models/basic_model.py:127-200 M3AEClassifier) and the two CAV-MAE branches (models/cav_mae.py:69-113,
116-186, 337-364; models/basic_model.py:202-275 Modal3Classifier, :79-124 CAVClassifier).

One `M3AEEncoder` per modality, like the reference's `mae_a` (text) / `mae_v` (image): pre-LN ViT-B
(emb 768, 12 heads, mlp x4) over [cls] + 256 tokens, token-mean feature.  DropPath == identity (SURVEY Q10:
the published DropPath returns None).  Same host design as the ResNet encoder: ONE flat fp32 buffer for the
parameters that receive gradients (Linear weights stored [in][out] = the GEMM B operand), one for gradients,
explicit forward/backward launch plans over a workspace allocated once; attention probabilities are kept
(not recomputed) for the backward.  Parameters the modality never touches (the image embedding of the text
encoder and vice versa) live outside the flat buffer: their gradient is None in the reference, so SGD skips them.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import MLAHipError
from .model import ConcatFusion, SharedHead, _Classifier, concat_fusion_forward
from .module import FlatEncoder
from .rows import RowPlan, check_present


def _sincos_1d(embed_dim: int, pos: np.ndarray) -> np.ndarray:                      # m3ae.py:181-194
    omega = np.arange(embed_dim // 2, dtype=np.float32)
    omega /= embed_dim / 2.
    omega = 1. / 10000 ** omega
    out = np.einsum('m,d->md', pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_pos_embed(embed_dim: int, length: int, two_d: bool) -> torch.Tensor:
    """get_1d_sincos_pos_embed / get_2d_sincos_pos_embed (m3ae.py:197-223), without the leading 1."""
    if not two_d:
        emb = _sincos_1d(embed_dim, np.arange(length, dtype=np.float32))
    else:
        gs = int(length ** 0.5)
        if gs * gs != length:
            raise MLAHipError("2-D position embedding needs a square patch grid")
        grid = np.stack(np.meshgrid(np.arange(gs, dtype=np.float32), np.arange(gs, dtype=np.float32)), axis=0)   # w first
        grid = grid.reshape([2, 1, gs, gs])
        emb = np.concatenate([_sincos_1d(embed_dim // 2, grid[0]), _sincos_1d(embed_dim // 2, grid[1])], axis=1)
    return torch.from_numpy(emb.astype(np.float32))


# measurement switch (same-box A/B): 0 = bias gradients by separate column-reduction launches
FUSE_BIAS_GRAD = os.environ.get("MLA_FUSE_BIAS_GRAD", "1") != "0"


# One row of an encoder's parameter table, all that is known about a trained parameter: internal name (key of layout / p / g),
# internal shape (Linear weights [in][out]), init rule ((shape, generator) -> initial value, drawn in table order), the
# reference-shaped VIEW of the internal tensor (no copy), and the reference state_dict key
_Param = namedtuple("_Param", "name shape init view ref")
_same = lambda t: t
_t = lambda t: t.t()                              # nn.Linear.weight is (out, in)
_row = lambda t: t.view(1, 1, -1)                 # type / modality embeddings and cls are (1, 1, D)
_lead = lambda t: t.view(1, *t.shape)             # learned position embedding (1, L, D)
# Conv2d(1 | 3, D, 16, 16) weight (cav_mae.py:80): patchify emits a patch as (c, p1, p2), the order of the conv weight's
# trailing dimensions, so splitting the transposed view's second dimension is all it takes
_conv16 = lambda t: t.t().view(t.shape[1], -1, 16, 16)

# The layers as forward / backward_from_pooled read them, bound once: parameter and gradient views (b / gb None without a
# bias), for a Linear also its [K][N] dims and the bf16 images its forward / input-gradient GEMMs read (None under "f32")
_Norm = namedtuple("_Norm", "w b gw gb")
_Linear = namedtuple("_Linear", "w b gw gb K N img_fwd img_dgrad")
_Block = namedtuple("_Block", "ln1 qkv fc ln2 fc1 fc2")
# ... and a block's layers in layout order: a LayerNorm, or a Linear with its (K, N) in units of D
_BLOCK_LAYERS = (("layer_norm1", None), ("attention.qkv_linear", (1, 3)), ("attention.fc", (1, 1)), ("layer_norm2", None),
                 ("transformer_mlp.fc1", (1, 4)), ("transformer_mlp.fc2", (4, 1)))


class M3AEEncoder(FlatEncoder):
    """nn.Module face (module.py): parameters under the reference's names, order and layouts -- nn.Linear weights
    (out, in) as transposed views of the [in][out] GEMM operands, type embeddings / cls as (1,1,D) -- registered as
    MaskedMultimodalAutoencoder does (direct parameters, text_embedding, image_embedding, encoder: m3ae.py:305-331)
    resp. the audio ("audio") or the visual ("cav_visual") branch of CAVMAEFT (cav_mae.py:116-145)."""

    def __init__(self, kind: str, device="cuda", depth: int = 12, emb_dim: int = 768, num_heads: int = 12,
                 text_vocab_size: int = 30522, patch_dim: int = 768, seed: Optional[int] = None, conv_math: Optional[str] = None,
                 attention_math: Optional[str] = None):
        if kind not in ("text", "image", "audio", "cav_visual"):
            raise ValueError("kind must be 'text', 'image', 'audio' or 'cav_visual'")
        super().__init__(device, conv_math)                  # conv_math: here the arithmetic of the Linear GEMMs
        self.split = self.conv_math in ("split", "bf16")      # both run on weight images and the fused bias gradient
        # "fused": one flash-style kernel per direction, scores never materialised (csrc/attention.hip); "materialized": the
        # round-1 form (QK^T -> masked softmax -> PV as strided batched GEMMs, probabilities kept in HBM), kept as a
        # cross-check of the fused kernels at full size and for A/B measurements
        self.attention = os.environ.get("MLA_ATTENTION", "fused")
        if self.attention not in ("fused", "materialized"):
            raise MLAHipError(f"MLA_ATTENTION must be 'fused' or 'materialized', got {self.attention!r}")
        # arithmetic of the fused kernels' five products: "f32" (fp32 MFMA, csrc/attention.hip) or "split" (exact three-way bf16
        # split, six products on the bf16 MFMA, csrc/attention_split.hip; same accuracy).  Independent of conv_math.
        self.attention_math = attention_math or os.environ.get("MLA_ATTENTION_MATH", "f32")
        if self.attention_math not in ops.ATTENTION_MATHS:
            raise MLAHipError(f"attention_math must be 'f32' or 'split', got {self.attention_math!r}")
        if self.attention_math == "split" and self.attention == "materialized":
            raise MLAHipError("attention_math='split' needs the fused attention kernels (MLA_ATTENTION=materialized is set)")
        self.kind = kind
        self.cav = kind in ("audio", "cav_visual")
        self.sfx = {"audio": "a", "cav_visual": "v"}.get(kind)       # CAVMAEFT's per-modality name suffix
        if kind == "audio":
            patch_dim = 256                  # conv 16x16 over 1 channel (cav_mae.py:126)
        elif kind == "cav_visual":
            patch_dim = 768                  # conv 16x16 over 3 channels (cav_mae.py:127)
        self.has_cls = not self.cav          # CAV-MAE has no [cls] token
        self.audio_tokens = 512              # audio_length * 128 / 256 (cav_mae.py:129)
        self.cav_tokens = {"audio": self.audio_tokens, "cav_visual": 196}.get(kind)      # 224 / 16 squared (cav_mae.py:75)
        self.depth, self.D, self.H, self.V, self.PD = depth, emb_dim, num_heads, text_vocab_size, patch_dim
        D = emb_dim
        # ---- the parameters this modality trains, in flat-buffer order
        self._table: Dict[str, _Param] = {r.name: r for r in self._param_table()}
        self._alloc_flat([(r.name, r.shape) for r in self._table.values()])
        # ---- parameters of the other modality's input path: never used, never receive a gradient (grad stays None, so
        # SGD skips them, like the reference); registered below with their own storage, reference shapes
        if kind == "text":
            unused_shapes = {"image_embedding.weight": (D, patch_dim), "image_embedding.bias": (D,),
                             "encoder_image_type_embedding": (1, 1, D)}
        elif kind == "image":
            unused_shapes = {"text_embedding.weight": (text_vocab_size, D), "encoder_text_type_embedding": (1, 1, D)}
        else:
            unused_shapes = {}   # CAVMAEFT's other branch / unused norms are not materialised (never touched by forward_feat)
        self.unused: Dict[str, nn.Parameter] = {}
        self._register_reference_tree(unused_shapes)
        self._ws: dict = {}                  # the workspace of the last forward: the planned one (_cap) or a prefix view of it
        self._key = None
        self._cap: Optional[dict] = None
        self._views: Dict[int, dict] = {}
        # split-bf16 images of every Linear weight ([K][N] = a 1-tap conv weight)
        self._build_wsplit([(k, k, 1) + shp for k, (_o, shp) in self.layout.items()
                            if len(shp) == 2 and k.endswith(".weight") and k != "text_embedding.weight"])
        # ---- every layer bound once: what one launch needs of it, as forward / backward_from_pooled read it
        self.embed = None if kind == "text" else self._bind(f"patch_embed_{self.sfx}.proj" if self.cav else "image_embedding")
        self._blocks = tuple(_Block(*(self._bind(f"encoder.blocks.{i}.{n}") for n, _kn in _BLOCK_LAYERS)) for i in range(depth))
        self._norm = self._bind("encoder.layer_norm")
        self.reset_parameters(seed)

    def _param_table(self) -> List[_Param]:
        """The per-kind parameter table.  Initialisation is the reference's module defaults (m3ae.py:306-324; nn.Linear /
        nn.LayerNorm defaults); reset_parameters draws in table order."""
        D, PD, x = self.D, self.PD, self.sfx
        uniform = lambda shp, gen: torch.rand(shp, generator=gen) * 2 - 1
        normal = lambda shp, gen: torch.randn(shp, generator=gen)

        def linear(name, K, N, bound=None, bias_fan=None, view=_t):   # nn.Linear default: weight and bias U(+-1/sqrt(fan_in))
            bound, bias_fan = bound or 1.0 / math.sqrt(K), bias_fan or K
            return [(name + ".weight", (K, N), lambda shp, gen: uniform(shp, gen) * bound, view),
                    (name + ".bias", (N,), lambda shp, gen: uniform(shp, gen) / math.sqrt(bias_fan), _same)]

        def layer_norm(name):
            return [(name + ".weight", (D,), lambda shp, gen: torch.ones(shp), _same),
                    (name + ".bias", (D,), lambda shp, gen: torch.zeros(shp), _same)]

        def type_embedding(name):                                     # torch.empty().normal_(0.02): mean .02, std 1
            return [(name, (D,), lambda shp, gen: normal(shp, gen) + 0.02, _row)]

        if self.kind == "text":
            rows = [("text_embedding.weight", (self.V, D), normal, _same)]                                   # normal_(0, 1)
            rows += type_embedding("encoder_text_type_embedding") + type_embedding("cls_token")
        elif self.kind == "image":
            rows = linear("image_embedding", PD, D, bound=math.sqrt(6.0 / (PD + D)))                         # xavier_uniform_
            rows += type_embedding("encoder_image_type_embedding") + type_embedding("cls_token")
        else:   # CAV-MAE: conv patch embed (as [256 | 768][D]), modality embedding, LEARNED position embedding (tr_pos=True)
            # (the conv bias is drawn with the block Linears' bound 1/sqrt(D), not 1/sqrt(PD): seeded weights depend on it)
            rows = linear(f"patch_embed_{x}.proj", PD, D, bias_fan=D, view=_conv16)
            rows += [(f"modality_{x}", (D,), lambda shp, gen: normal(shp, gen) * 0.02, _row),               # cav_mae.py:172-173
                     (f"pos_embed_{x}", (self.cav_tokens, D), lambda shp, gen: self._cav_pos_embed(), _lead)]   # :161-165
        for i in range(self.depth):
            for n, kn in _BLOCK_LAYERS:
                name = f"encoder.blocks.{i}.{n}"
                rows += layer_norm(name) if kn is None else linear(name, kn[0] * D, kn[1] * D)
        rows += layer_norm("encoder.layer_norm")
        return [_Param(*r, self._ref_name(r[0])) for r in rows]

    def _bind(self, name: str):
        """The layer `name` as the launches read it: a _Norm, or for a 2-D weight a _Linear."""
        w, b = name + ".weight", name + ".bias"
        if len(self.layout[w][1]) == 1:
            return _Norm(self.p[w], self.p[b], self.g[w], self.g[b])
        return _Linear(self.p[w], self.p.get(b), self.g[w], self.g.get(b), *self.layout[w][1], *self.wsp.get(w, (None, None)))

    # ---- reference-named parameter tree -----------------------------------------------------------
    def _to_ref(self, name: str):
        """internal flat view -> reference-shaped VIEW (no copy)."""
        return self._table[name].view

    def _register_reference_tree(self, unused_shapes: Dict[str, Tuple[int, ...]]) -> None:
        if self.cav:
            x = self.sfx
            order = [f"modality_{x}", f"pos_embed_{x}", f"patch_embed_{x}.proj.weight", f"patch_embed_{x}.proj.bias"]
        else:
            order = ["encoder_image_type_embedding", "encoder_text_type_embedding", "cls_token", "text_embedding.weight",
                     "image_embedding.weight", "image_embedding.bias"]
        order += [k for k in self.layout if k.startswith("encoder.")]
        for name in order:
            row = self._table.get(name)
            if row is not None:
                p = self._param_view(self.p[name], self.g[name], row.view, row.ref)
            else:
                p = nn.Parameter(torch.zeros(unused_shapes[name], device=self.device, dtype=torch.float32))
                p._mla_owner = self
                self.unused[name] = p
            parent, leaf = self._descend(self, self._ref_name(name))
            parent.register_parameter(leaf, p)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset_parameters(self, seed: Optional[int] = None) -> None:
        """Module-default initialisation of the reference, as the parameter table states it."""
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed) if seed is not None else gen.seed()
        for r in self._table.values():
            self.p[r.name].copy_(r.init(r.shape, gen))

    def _cav_pos_embed(self) -> torch.Tensor:
        """get_2d_sincos_pos_embed(D, 8, L/8) (audio) / (D, 14, 14) (visual) of cav_mae.py:51-66, 161-165 ('w goes first')."""
        D, L = self.D, self.cav_tokens
        gh, gw = (8, L // 8) if self.kind == "audio" else (14, 14)
        grid = np.stack(np.meshgrid(np.arange(gw, dtype=np.float32), np.arange(gh, dtype=np.float32)), axis=0).reshape([2, 1, gw, gh])
        emb = np.concatenate([_sincos_1d(D // 2, grid[0]), _sincos_1d(D // 2, grid[1])], axis=1)
        return torch.from_numpy(emb.astype(np.float32))

    def _ref_name(self, name: str) -> str:
        """internal (M3AE-style) parameter name -> reference state_dict key."""
        if not self.cav or not name.startswith("encoder."):
            return name
        x = self.sfx
        if name.startswith("encoder.layer_norm."):
            return name.replace("encoder.layer_norm.", f"norm_{x}.")                       # cav_mae.py:142-143, 350, 363
        _e, _b, i, rest = name.split(".", 3)
        i = int(i)
        shared = i >= self.depth - 1                                             # 11 blocks_a|v + 1 blocks_u (cav_mae.py:138-140)
        pre = f"blocks_u.{i - (self.depth - 1)}." if shared else f"blocks_{x}.{i}."
        sub = {"layer_norm1": f"norm1_{x}" if shared else "norm1", "layer_norm2": f"norm2_{x}" if shared else "norm2",
               "attention.qkv_linear": "attn.qkv", "attention.fc": "attn.proj", "transformer_mlp.fc1": "mlp.fc1",
               "transformer_mlp.fc2": "mlp.fc2"}
        for k, v in sub.items():
            if rest.startswith(k + "."):
                return pre + v + rest[len(k):]
        raise KeyError(name)

    def grads_as_reference(self) -> Dict[str, torch.Tensor]:
        return {r.ref: r.view(self.g[r.name]).clone(memory_format=torch.contiguous_format) for r in self._table.values()}

    # ------------------------------------------------------------------------------------------
    def _plan(self, B: int, L: int) -> dict:
        """The workspace of a forward on B samples of L tokens.  Buffers are allocated once, at the largest batch seen so far (or
        at reserve()'s): every one is row-major in M = B n or (B, H, n), so a smaller batch runs in a prefix of the same
        memory, through views that are made once per B.  Only a batch larger than any before (or another L) allocates again."""
        if self._key == (B, L):
            return self._ws
        cap = self._cap
        if cap is None or cap["L"] != L or B > cap["B"]:
            cap, self._views = self._alloc_ws(B, L), {}
            self._cap = cap
        if B == cap["B"]:
            ws = cap
        else:
            ws = self._views.get(B)
            if ws is None:
                ws = self._views[B] = self._prefix_ws(cap, B)
        self._ws, self._key = ws, (B, L)
        return ws

    def reserve(self, B: int, L: int, backward: bool = True) -> None:
        """Allocate the workspace for batches of up to B samples of L tokens now (and, with `backward`, the backward's), so that no
        later batch of at most B samples allocates any of it."""
        cap = self._cap
        if cap is None or cap["L"] != L or B > cap["B"]:
            self._plan(B, L)
        if backward:
            self._bwd_ws(self._cap)

    def workspace_tensors(self) -> Dict[str, torch.Tensor]:
        """path -> buffer of the planned workspace (the allocation that batches up to its size run in), without what a forward
        leaves beside them: the padding mask it builds and the aliases "x" / "xlast"."""
        def walk(path, v):
            if isinstance(v, torch.Tensor):
                yield path, v
            elif isinstance(v, dict):
                for k, x in v.items():
                    if k not in ("pm", "x", "xlast"):
                        yield from walk(f"{path}.{k}", x)
            elif isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    yield from walk(f"{path}[{i}]", x)
        return dict(walk("ws", self._cap or {}))

    def _prefix_ws(self, cap: dict, B: int) -> dict:
        """The planned workspace `cap` cut to its first B samples: views, no memory of its own."""
        L, n = cap["L"], cap["n"]
        M = B * n
        ws: dict = {"B": B, "L": L, "n": n, "M": M, "cap": cap, "x0": cap["x0"][:M], "y": cap["y"][:M], "feat": cap["feat"][:B],
                    "stf": [r[:M] for r in cap["stf"]], "blocks": []}
        for bk in cap["blocks"]:
            v = {k: bk[k][:M] for k in ("h1", "qkv", "o", "xmid", "h2", "u", "gl", "xout")}
            v["st"] = [r[:M] for r in bk["st"]]
            for k in ("P", "lse"):
                if k in bk:
                    v[k] = bk[k][:B]
            ws["blocks"].append(v)
        if "patches" in cap:
            ws["patches"] = cap["patches"][:B * L]
        if "pos" in cap:
            ws["pos"] = cap["pos"]
        if "ids" in cap:
            ws["ids"] = cap["ids"][:B]
        return ws

    def _scratch(self, ws: dict, name: str, elems: int, dtype=torch.float32) -> torch.Tensor:
        """ws[name], a scratch buffer of at least `elems` elements: the planned workspace's where that one is large enough."""
        if name not in ws:
            have = ws["cap"].get(name) if "cap" in ws else None
            ws[name] = have if have is not None and have.numel() >= elems else torch.empty(elems, device=self.device, dtype=dtype)
        return ws[name]

    def _alloc_ws(self, B: int, L: int) -> dict:
        D, H, n = self.D, self.H, L + (1 if self.has_cls else 0)
        M = B * n
        f32 = dict(device=self.device, dtype=torch.float32)
        ws: dict = {"B": B, "L": L, "n": n, "M": M}
        ws["x0"] = torch.empty((M, D), **f32)
        ws["blocks"] = []
        for _ in range(self.depth):
            ws["blocks"].append({"h1": torch.empty((M, D), **f32), "qkv": torch.empty((M, 3 * D), **f32),
                                 "P": torch.empty((B, H, n, n), **f32), "o": torch.empty((M, D), **f32),
                                 "xmid": torch.empty((M, D), **f32), "h2": torch.empty((M, D), **f32),
                                 "u": torch.empty((M, 4 * D), **f32), "gl": torch.empty((M, 4 * D), **f32),
                                 "xout": torch.empty((M, D), **f32),
                                 "st": torch.empty((4, M), **f32)})          # mean1, rstd1, mean2, rstd2
        ws["y"] = torch.empty((M, D), **f32)
        ws["stf"] = torch.empty((2, M), **f32)
        ws["feat"] = torch.empty((B, D), **f32)
        if self.kind != "text":
            ws["patches"] = torch.empty((B * L, self.PD), **f32)
        else:   # owned copy of the token ids: tokens_assemble_bwd reads it after forward() returned (feeder slots are reused)
            ws["ids"] = torch.empty((B, L), device=self.device, dtype=torch.int64)
        if not self.cav:
            ws["pos"] = sincos_pos_embed(D, L, two_d=(self.kind == "image")).to(self.device)
        if self.attention == "fused":
            for bk in ws["blocks"]:
                del bk["P"]
                bk["lse"] = torch.empty((B, H, n), **f32)
        return ws

    def _bwd_ws(self, ws: dict) -> None:
        if "dA" in ws:
            return
        D, H, n, M, B = self.D, self.H, ws["n"], ws["M"], ws["B"]
        f32 = dict(device=self.device, dtype=torch.float32)
        cap = ws.get("cap")
        if cap is None:
            ws["dA"], ws["dB"], ws["dC"] = (torch.empty((M, D), **f32) for _ in range(3))
            ws["du"] = torch.empty((M, 4 * D), **f32)
            ws["dqkv"] = torch.empty((M, 3 * D), **f32)
            if self.attention == "fused":
                ws["dvec"] = torch.empty((B, H, n), **f32)
            else:
                ws["dP"] = torch.empty((B, H, n, n), **f32)
            ws["wt_ws"] = torch.empty(4 * D * D, **f32)
            ws["colsum"] = torch.empty(D, **f32)
        else:   # a prefix of the planned workspace's (sizes that do not depend on the batch: the buffers themselves)
            self._bwd_ws(cap)
            for k in ("dA", "dB", "dC", "du", "dqkv"):
                ws[k] = cap[k][:M]
            for k in ("dvec", "dP"):
                if k in cap:
                    ws[k] = cap[k][:B]
            ws["wt_ws"], ws["colsum"] = cap["wt_ws"], cap["colsum"]
        # one weight-gradient workspace: the largest any bound Linear asks for at the rows it really runs on
        gemms = {(M, lin.K, lin.N) for blk in self._blocks for lin in (blk.qkv, blk.fc, blk.fc1, blk.fc2)}
        if self.embed is not None:
            gemms.add((B * ws["L"], self.embed.K, self.embed.N))
        wb = max(ops.linear_wgrad_ws_bytes(*mkn, sp, sp and self.bf16) for sp in ((False, True) if self.split else (False,))
                 for mkn in gemms)
        self._scratch(ws, "wgrad_ws", (wb + 3) // 4)
        self._scratch(ws, "red_ws", ops.colreduce_ws_elems(M, 4 * D))

    # ---- the Linear launches: the only callers of ops.linear_* here; arithmetic flags and weight image come from the encoder
    def _lin_fwd(self, lin: _Linear, x, y, rows: int, st, groups: int = 1, y_group_rows: Optional[int] = None, y_off: int = 0,
                 residual=None, y_gelu=None) -> None:
        ops.linear_fwd(x, lin.w, lin.b, y, groups, rows, lin.K, lin.N, y_group_rows=y_group_rows, y_off=y_off, residual=residual,
                       y_gelu=y_gelu, stream=st, bf16=self.bf16, wsplit=lin.img_fwd)

    def _lin_dgrad(self, lin: _Linear, dy, dx, rows: int, ws: dict, st, gelu_src=None) -> None:
        ops.linear_dgrad(dy, lin.w, dx, ws["wt_ws"], 1, rows, lin.K, lin.N, gelu_src=gelu_src, stream=st, bf16=self.bf16,
                         wsplit=lin.img_dgrad)

    def _lin_wgrad(self, lin: _Linear, x, dy, rows: int, ws: dict, st, bias: bool = True) -> None:
        """Weight gradient of one Linear (dw = x^T dy) and, with `bias`, its bias gradient (db = column sums of dy).  On the
        weight-image arithmetics the bias gradient comes out of the weight-gradient kernel's own pass over dy; otherwise
        (fp32, or FUSE_BIAS_GRAD off) from a column reduction launched first."""
        fused = bias and self.split and FUSE_BIAS_GRAD
        if bias and not fused:
            ops.colsum_rows(dy, lin.gb, ws["red_ws"], rows, lin.N, stream=st)
        ops.linear_wgrad(x, dy, lin.gw, ws["wgrad_ws"], 1, rows, lin.K, lin.N, stream=st, split=self.split,
                         dbias=lin.gb if fused else None, bf16=self.bf16)

    def tokens(self, inp: torch.Tensor) -> int:
        """L, the tokens per sample (without [cls]) that forward() makes of `inp`: what reserve() is told."""
        if self.kind == "text":
            return inp[0].numel()
        if self.kind == "audio":
            return (inp.shape[2] // 16) * (inp.shape[1] // 16)
        return (inp.shape[2] // 16) * (inp.shape[3] // 16)

    # ------------------------------------------------------------------------------------------
    def forward(self, inp: torch.Tensor, padding_mask: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """text: inp = token ids (B,1,L) or (B,L) int64, padding_mask (B,1,L)/(B,L) float (1 = padded);
        image: inp = (B,3,256,256) fp32; audio: inp = (B,1024,128) fp32; cav_visual: inp = (B,3,224,224) fp32.
        Returns the (B, D) token-mean feature (basic_model.py:182-200), written into `out` if given (else into the reused
        workspace buffer)."""
        self._await_tail()
        st = ops.cur_stream()
        D, H = self.D, self.H
        hd = D // H
        if self.split and (self.training or self._wsplit_dirty):
            self._refresh_wsplit(st)
        if self.kind == "text":
            ids = inp.reshape(inp.shape[0], -1).contiguous()                                 # token.squeeze(1)
            B, L = ids.shape
            ws = self._plan(B, L)
            pm = padding_mask.reshape(B, -1).to(torch.float32)
            ws["ids"].copy_(ids)     # owned copy: tokens_assemble_bwd reads it after forward() returned (feeder slots are reused)
            ids = ws["ids"]
            # cls is never masked (m3ae.py:347)
            ws["pm"] = torch.cat([torch.zeros((B, 1), device=self.device), pm], dim=1).contiguous()
            ops.tokens_assemble(ws["x0"], self.p["text_embedding.weight"], ids, ws["pos"], self.p["encoder_text_type_embedding"],
                                self.p["cls_token"], B, L, D, stream=st)
        else:
            transposed_hw = None
            if self.kind == "audio":
                # cav_mae.py:337-343: (B, time, freq) -> unsqueeze, transpose -> conv16x16/16 -> (B, 8*64, D) + pos + modality
                B, T_, F_ = inp.shape
                L = (F_ // 16) * (T_ // 16)
                if L != self.audio_tokens:
                    raise MLAHipError(f"audio encoder expects {self.audio_tokens} patches, got {L}")
                transposed_hw = (F_, T_)
            elif self.kind == "cav_visual":
                # cav_mae.py:352-355: conv16x16/16 over (B, 3, 224, 224) -> (B, 14*14, D) + pos_embed_v + modality_v
                if inp.dim() != 4 or inp.shape[1] != 3 or (inp.shape[2] // 16) * (inp.shape[3] // 16) != self.cav_tokens:
                    raise MLAHipError(f"cav_visual encoder expects (B, 3, 224, 224), got {tuple(inp.shape)}")
                B, L = inp.shape[0], self.cav_tokens
            else:
                B = inp.shape[0]
                L = (inp.shape[2] // 16) * (inp.shape[3] // 16)
            ws = self._plan(B, L)
            ws["pm"] = None
            img = inp.contiguous().float() if self.cav else inp.contiguous()
            ops.patchify(img, ws["patches"], 16, transposed_hw=transposed_hw, stream=st)     # basic_model.py:184-186
            if self.cav:
                self._lin_fwd(self.embed, ws["patches"], ws["x0"], B * L, st)
                ops.tokens_assemble(ws["x0"], None, None, self.p[f"pos_embed_{self.sfx}"], self.p[f"modality_{self.sfx}"], None,
                                    B, L, D, stream=st)
            else:   # the patch rows land behind each sample's [cls] row (m3ae.py:353)
                self._lin_fwd(self.embed, ws["patches"], ws["x0"], L, st, groups=B, y_group_rows=L + 1, y_off=1)
                ops.tokens_assemble(ws["x0"], None, None, ws["pos"], self.p["encoder_image_type_embedding"], self.p["cls_token"],
                                    B, L, D, stream=st)
        n, M = ws["n"], ws["M"]
        scale = hd ** -0.5
        x = ws["x0"]
        for blk, bk in zip(self._blocks, ws["blocks"]):
            bk["x"] = x
            ops.layernorm_fwd(x, blk.ln1.w, blk.ln1.b, bk["h1"], bk["st"][0], bk["st"][1], M, D, stream=st)
            self._lin_fwd(blk.qkv, bk["h1"], bk["qkv"], M, st)
            if self.attention == "fused":
                ops.attention_fwd(bk["qkv"], ws["pm"], bk["o"], bk["lse"], B, H, n, hd, stream=st, math=self.attention_math)   # m3ae.py:109-122
            else:   # element strides (batch, head, row, col) of q | k | v inside qkv, of k^T, of the scores, of o
                qs, kt, os_ = (n * 3 * D, hd, 3 * D, 1), (n * 3 * D, hd, 1, 3 * D), (n * D, hd, D, 1)
                ss = (H * n * n, n * n, n, 1)
                ops.bgemm(bk["qkv"], bk["qkv"], bk["P"], B, H, n, n, hd, qs, kt, ss, scale, b_off=D, stream=st)   # m3ae.py:109
                ops.softmax_fwd(bk["P"], ws["pm"], B, H, n, stream=st)                                            # :111-118
                ops.bgemm(bk["P"], bk["qkv"], bk["o"], B, H, n, hd, n, ss, qs, os_, 1.0, b_off=2 * D, stream=st)  # :121-122
            self._lin_fwd(blk.fc, bk["o"], bk["xmid"], M, st, residual=x)                                     # :123,149
            ops.layernorm_fwd(bk["xmid"], blk.ln2.w, blk.ln2.b, bk["h2"], bk["st"][2], bk["st"][3], M, D, stream=st)
            self._lin_fwd(blk.fc1, bk["h2"], bk["u"], M, st, y_gelu=bk["gl"])                                 # :76-77
            self._lin_fwd(blk.fc2, bk["gl"], bk["xout"], M, st, residual=bk["xmid"])                          # :79,154
            x = bk["xout"]
        ws["xlast"] = x
        ops.layernorm_fwd(x, self._norm.w, self._norm.b, ws["y"], ws["stf"][0], ws["stf"][1], M, D, stream=st)   # m3ae.py:176
        feat = ws["feat"] if out is None else out
        ops.avgpool_fwd(ws["y"], feat, B, n, D, stream=st)                                    # .mean(dim=1) over all 1+L tokens
        self._pa = n
        return feat

    # ------------------------------------------------------------------------------------------
    def backward_from_pooled(self, dfeat: torch.Tensor, P: Optional[int] = None) -> None:
        ws = self._ws
        self._bwd_ws(ws)
        st = ops.cur_stream()
        D, H, n, M, B, L = self.D, self.H, ws["n"], ws["M"], ws["B"], ws["L"]
        hd = D // H
        scale = hd ** -0.5
        dA, dB_, dC = ws["dA"], ws["dB"], ws["dC"]
        red = ws["red_ws"]
        ops.avgpool_bwd(dfeat.contiguous(), dA, B, n, D, stream=st)                                             # d y
        ops.layernorm_bwd(dA, ws["xlast"], self._norm.w, ws["stf"][0], ws["stf"][1], dA, self._norm.gw, self._norm.gb, red, M, D,
                          stream=st)
        dx = dA                                                                                            # grad wrt block output
        for blk, bk in zip(reversed(self._blocks), reversed(ws["blocks"])):
            # ---- MLP: xout = xmid + fc2(gelu(fc1(LN2(xmid))))
            self._lin_wgrad(blk.fc2, bk["gl"], dx, M, ws, st)
            self._lin_dgrad(blk.fc2, dx, ws["du"], M, ws, st, gelu_src=bk["u"])
            self._lin_wgrad(blk.fc1, bk["h2"], ws["du"], M, ws, st)
            self._lin_dgrad(blk.fc1, ws["du"], dB_, M, ws, st)                                                  # d h2
            ops.layernorm_bwd(dB_, bk["xmid"], blk.ln2.w, bk["st"][2], bk["st"][3], dB_, blk.ln2.gw, blk.ln2.gb, red, M, D,
                              add=dx, stream=st)                                                                # d xmid -> dB_
            # ---- attention: xmid = x + fc(PV)
            self._lin_wgrad(blk.fc, bk["o"], dB_, M, ws, st)
            self._lin_dgrad(blk.fc, dB_, dC, M, ws, st)                                                         # d o (B,n,D)
            if self.attention == "fused":
                ops.attention_bwd(dC, bk["qkv"], bk["o"], bk["lse"], ws["pm"], ws["dqkv"], ws["dvec"], B, H, n, hd, stream=st,
                                  math=self.attention_math)
            else:
                qs, kt, os_ = (n * 3 * D, hd, 3 * D, 1), (n * 3 * D, hd, 1, 3 * D), (n * D, hd, D, 1)       # as in forward
                ss, sT = (H * n * n, n * n, n, 1), (H * n * n, n * n, 1, n)                                  # scores, scores^T
                ops.bgemm(dC, bk["qkv"], ws["dP"], B, H, n, n, hd, os_, kt, ss, 1.0, b_off=2 * D, stream=st)        # dP = dO V^T
                ops.bgemm(bk["P"], dC, ws["dqkv"], B, H, n, hd, n, sT, os_, qs, 1.0, c_off=2 * D, stream=st)        # dV = P^T dO
                ops.softmax_bwd(bk["P"], ws["dP"], B, H, n, stream=st)                                              # dS
                ops.bgemm(ws["dP"], bk["qkv"], ws["dqkv"], B, H, n, hd, n, ss, qs, qs, scale, b_off=D, stream=st)   # dQ = s dS K
                ops.bgemm(ws["dP"], bk["qkv"], ws["dqkv"], B, H, n, hd, n, sT, qs, qs, scale, c_off=D, stream=st)  # dK = s dS^T Q
            self._lin_wgrad(blk.qkv, bk["h1"], ws["dqkv"], M, ws, st)
            self._lin_dgrad(blk.qkv, ws["dqkv"], dC, M, ws, st)                                                 # d h1
            ops.layernorm_bwd(dC, bk["x"], blk.ln1.w, bk["st"][0], bk["st"][1], dC, blk.ln1.gw, blk.ln1.gb, red, M, D,
                              add=dB_, stream=st)                                                               # d x -> dC
            dx, dC = dC, dx                                                                                     # rotate buffers
            ws["dA"], ws["dC"] = dx, dC
        # ---- token assembly (m3ae.py:342-366)
        ops.colsum_rows(dx, ws["colsum"], red, M, D, stream=st)
        if self.cav:
            # x0 = conv(patches) + pos_embed + modality: d modality = d conv-bias = sum over all tokens,
            # d pos[i] = sum over the batch, d conv-weight = patches^T dx
            self.g[f"modality_{self.sfx}"].copy_(ws["colsum"])
            self.embed.gb.copy_(ws["colsum"])
            ops.colsum_rows(dx, self.g[f"pos_embed_{self.sfx}"], self._scratch(ws, "red_pos", ops.colreduce_ws_elems(B, L * D)), B, L * D,
                            stream=st)
            self._lin_wgrad(self.embed, ws["patches"], dx, B * L, ws, st, bias=False)
        elif self.kind == "text":
            self.g["text_embedding.weight"].zero_()
            emb_ws = self._scratch(ws, "emb_ws", ops.tokens_assemble_bwd_ws_bytes(B, L, D), torch.uint8)
            ops.tokens_assemble_bwd(dx, ws["colsum"], ws["ids"], self.g["cls_token"], self.g["encoder_text_type_embedding"],
                                    self.g["text_embedding.weight"], B, L, D, stream=st, ws=emb_ws)
        else:
            ops.tokens_assemble_bwd(dx, ws["colsum"], None, self.g["cls_token"], self.g["encoder_image_type_embedding"], None,
                                    B, L, D, stream=st)
            # the embed's bias gradient sums the patch rows only, so it is reduced here and not inside the weight gradient
            dimg = dx.view(B, n, D)[:, 1:, :].contiguous().view(B * L, D)       # memory plumbing: drop the cls rows
            ops.colsum_rows(dimg, self.embed.gb, red, B * L, D, stream=st)
            self._lin_wgrad(self.embed, ws["patches"], dimg, B * L, ws, st, bias=False)


class M3AEClassifier(_Classifier):
    """models/basic_model.py:127-200: mae_a (text) + mae_v (image) + ConcatFusion: Linear(768, C) shared (--gs_flag) or
    Linear(1536, C) on cat(a, v) (:149-152).  forward returns (a, v) either way: the reference loop calls
    fusion_module(a, v) itself (main.py:236-237)."""

    def __init__(self, args, device="cuda", depth: int = 12, text_vocab_size: int = 30522, seed: Optional[int] = None,
                 conv_math: Optional[str] = None, attention_math: Optional[str] = None):
        super().__init__(args, device, seed, ("Food101", "MVSA", "CREMAD"), ConcatFusion, 768, 2)             # :132-163
        kw = dict(depth=depth, text_vocab_size=text_vocab_size, conv_math=conv_math, attention_math=attention_math)
        self.mae_a = M3AEEncoder("text", device, seed=self._seed(0), **kw)                                    # :166
        self.mae_v = M3AEEncoder("image", device, seed=self._seed(1), **kw)                                   # :167

    def mla_encoders(self):
        return [("a", "text", self.mae_a), ("v", "image", self.mae_v)]

    def _calls(self, token: torch.Tensor, padding_mask: torch.Tensor, visual: torch.Tensor):
        """a, v = model(token, padding_mask, image)  (main.py:426; basic_model.py:182-200)"""
        return visual.shape[0], [lambda out=None: self.mae_a.forward(token, padding_mask, out),
                                 lambda out=None: self.mae_v.forward(visual, None, out)]


class ConcatFusion3(nn.Module):
    """models/fusion_modules.py:26-35.  Under --gs_flag (joint=False) only `fc_out` is touched (main.py:432, 444, 456) and
    forward raises; the joint step calls forward(x, y, z) -> (x, y, z, fc_out(cat(x, y, z))) (main.py:232-233)."""

    def __init__(self, input_dim: int = 768, output_dim: int = 4, device="cuda", seed: Optional[int] = None,
                 joint: bool = False):
        super().__init__()
        self.joint = bool(joint)
        self.fc_out = SharedHead(input_dim, output_dim, device, seed)

    def forward(self, x, y, z):
        return concat_fusion_forward(self, (x, y, z))


class Modal3Classifier(_Classifier):
    """models/basic_model.py:202-275: CAV-MAE audio (mae_a) + M3AE image (mae_v) + M3AE text (mae_t), head Linear(768, 4)
    shared (--gs_flag) or Linear(2304, 4) on cat(a, v, t) (:218-221); MLA alternates a -> v -> t (main.py:432-466).

    `present=` (forward, forward_raw, forward_split; MLATrainer.train_step and Evaluator.update pass it on): a HOST bool / uint8
    tensor (B, 3), columns (audio, image, text) as in Modal3Batcher(mask=) -- Modal3Batcher.present(step) -- that says which
    modalities each sample has; the inputs of the others must be what the batcher leaves there, zeros.  Each encoder then runs on
    its modality's P present rows plus one zero row instead of all B (mla_hip.rows), which in exact arithmetic is the same step:
    these encoders have no BatchNorm and no dropout, so every absent sample has the feature f(0).  The result differs from the
    call without `present` in the order of floating-point sums only.  A modality that every sample has takes the path without
    `present`, launch for launch.  Not offered by JointTrainer / QMFTrainer, nor by M3AEClassifier, CAVClassifier and
    AVClassifier: the reference masks modalities for IEMOCAP only, and AVClassifier's ResNets have BatchNorm, whose batch
    statistics make a sample's feature depend on every other row, zeros included."""

    def __init__(self, args, device="cuda", depth: int = 12, text_vocab_size: int = 30522, seed: Optional[int] = None,
                 conv_math: Optional[str] = None, attention_math: Optional[str] = None):
        super().__init__(args, device, seed, ("IEMOCAP",), ConcatFusion3, 768, 3)                             # :208-229
        self._row_bufs: Dict[tuple, torch.Tensor] = {}
        kw = dict(depth=depth, text_vocab_size=text_vocab_size, conv_math=conv_math, attention_math=attention_math)
        self.mae_a = M3AEEncoder("audio", device, depth=depth, seed=self._seed(0), conv_math=conv_math,       # :231 CAVMAEFT
                                 attention_math=attention_math)
        self.mae_v = M3AEEncoder("image", device, seed=self._seed(1), **kw)                                   # :232
        self.mae_t = M3AEEncoder("text", device, seed=self._seed(2), **kw)                                    # :233

    def mla_encoders(self):
        return [("a", "audio", self.mae_a), ("v", "image", self.mae_v), ("t", "text", self.mae_t)]

    def _calls(self, token, padding_mask, visual, audio, present=None):
        """a, v, t = model(token, padding_mask, image, spec)  (main.py:424; basic_model.py:252-275); with `present`, each encoder
        on the rows that have its modality (class docstring)."""
        B = visual.shape[0]
        inputs = (("a", self.mae_a, (audio,)), ("v", self.mae_v, (visual,)), ("t", self.mae_t, (token, padding_mask)))
        have = None if present is None else check_present(present, B, len(inputs))
        runs = []
        for k, (tag, enc, xs) in enumerate(inputs):
            if have is None or bool(have[:, k].all()):
                runs.append(self._run_all(enc, xs))
            else:
                runs.append(self._run_present(tag, enc, xs, RowPlan(have[:, k])))
        return B, runs

    @staticmethod
    def _run_all(enc, xs):
        def run(out=None):
            enc._row_grad = None                         # the backward takes the (B, D) feature gradient as it is
            return enc.forward(xs[0], xs[1] if len(xs) > 1 else None, out)
        return run

    def _row_buf(self, tag: str, name, shape, dtype=torch.float32) -> torch.Tensor:
        key = (tag, name, tuple(shape), dtype)
        if key not in self._row_bufs:
            self._row_bufs[key] = torch.empty(tuple(shape), device=self.device, dtype=dtype)
        return self._row_bufs[key]

    def _run_present(self, tag: str, enc, xs, plan: RowPlan):
        """The forward of one encoder on its plan.P present rows and one zero row; leaves the matching compaction of the feature
        gradient on the encoder (rows.compact_feature_grad).  Everything is enqueued on the stream run() is called on."""
        def run(out=None):
            B, rows, D = plan.B, plan.rows, self.feat_dim
            plan.upload(self._row_buf(tag, "tables", (2 * B,), torch.int64))
            packed = []
            for j, x in enumerate(xs):
                x = (x if x.dtype in (torch.float32, torch.int64) else x.float()).contiguous()
                dst = self._row_buf(tag, j, x.shape, x.dtype)[:rows]
                packed.append(ops.rows_gather(x, plan.idx, plan.idx_host, dst, zero_tail_rows=1))
            enc.reserve(B, enc.tokens(packed[0]), backward=False)        # the workspace every later batch of <= B rows runs in
            feat = enc.forward(packed[0], packed[1] if len(packed) > 1 else None, self._row_buf(tag, "feat", (B, D))[:rows])
            if out is None:
                out = self._row_buf(tag, "out", (B, D))
            ops.rows_expand(feat, plan.map, plan.map_host, out)
            dfeat_rows = self._row_buf(tag, "dfeat", (B, D))[:rows]
            enc._row_grad = lambda dfeat: ops.rows_compact_sum(dfeat.contiguous(), plan.idx, plan.idx_host, plan.absent, plan.absent_host,
                                                               dfeat_rows)
            return out
        return run


class CAVClassifier(_Classifier):
    """models/basic_model.py:79-124 (`--lorb large`): two CAV-MAE ViT-B encoders -- mae_a runs CAVMAEFT's audio branch, mae_v its
    visual branch (forward_feat(., 'a') / (., 'v'), cav_mae.py:337-364); the other branch of each CAVMAEFT is never touched and
    not materialised -- and ConcatFusion: Linear(768, 6) shared (--gs_flag) or Linear(1536, 6) on cat(a, v) (:95-98).  forward
    returns (a, v), the token means (:119-124), either way: the reference's large model has no fused forward, main.py:541-542
    applies fusion_module outside it.

    audio_ckpt / visual_ckpt stand for the reference's hard-coded "/path/to/cavmae-*.pth" (:109-117): each a CAVMAEFT state
    dict, loaded non-strictly -- the keys of the branch that is not materialised are ignored; None keeps the seeded
    initialisation."""
    lorb_large = True

    def __init__(self, args, device="cuda", depth: int = 12, seed: Optional[int] = None, conv_math: Optional[str] = None,
                 audio_ckpt: Optional[str] = None, visual_ckpt: Optional[str] = None, attention_math: Optional[str] = None):
        super().__init__(args, device, seed, ("CREMAD",), ConcatFusion, 768, 2)                               # :82-104
        kw = dict(depth=depth, conv_math=conv_math, attention_math=attention_math)
        self.mae_a = M3AEEncoder("audio", device, seed=self._seed(0), **kw)                                   # :106
        self.mae_v = M3AEEncoder("cav_visual", device, seed=self._seed(1), **kw)                              # :107
        for enc, path in ((self.mae_a, audio_ckpt), (self.mae_v, visual_ckpt)):                               # :109-117
            if path is not None:
                enc.load_state_dict(torch.load(path, map_location="cpu"), strict=False)   # other-branch keys: unexpected, ignored

    def mla_encoders(self):
        return [("a", "audio", self.mae_a), ("v", "visual", self.mae_v)]

    def _calls(self, audio: torch.Tensor, visual: torch.Tensor):
        """a, v = model(spec, image)  (main.py:420; basic_model.py:119-124): spec (B, 1024, 128), image (B, 3, 224, 224)"""
        if visual.shape[0] != audio.shape[0]:
            raise MLAHipError("audio/visual batch mismatch")
        return audio.shape[0], [lambda out=None: self.mae_a.forward(audio, None, out),
                                lambda out=None: self.mae_v.forward(visual, None, out)]
