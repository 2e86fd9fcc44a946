"""CPU restatement of the reference's `--lorb large` family for the tests: the visual branch of CAVMAEFT
(models/cav_mae.py:352-364), CAVClassifier (models/basic_model.py:79-124), the --cav_opti parameter groups (main.py:739-747) and
one MLA iteration of main.py:419-476 under torch.optim.Adam.

PARITY UNPINNED against the reference binary, like the audio branch (oracle/mla_oracle.py, cavmae_audio_feature): timm==0.4.5
(Attention / Mlp) is neither vendored nor installed, so the blocks restate cav_mae.py:86-113 plus timm 0.4.5's published
definitions: Attention = qkv Linear (bias) -> (B, N, 3, H, hd) -> softmax(q k^T * hd^-0.5) v -> proj Linear; Mlp = fc1 ->
GELU(erf) -> fc2."""
from typing import Dict, List

import torch
import torch.nn.functional as F

from oracle import mla_oracle as O

BLOCK = ["attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
         "mlp.fc2.bias"]


def branch_param_names(x: str, depth: int = 12) -> List[str]:
    """state_dict keys of the branch `x` ('a' | 'v') of CAVMAEFT that forward_feat(., x) touches, in the module's registration order
    (cav_mae.py:126-143: modality, pos_embed, patch_embed, blocks_x, blocks_u, norm_x; Block: norm1*, attn, norm2*, mlp)."""
    names = [f"modality_{x}", f"pos_embed_{x}", f"patch_embed_{x}.proj.weight", f"patch_embed_{x}.proj.bias"]
    for i in range(depth):
        shared = i >= depth - 1
        pre = f"blocks_u.{i - (depth - 1)}." if shared else f"blocks_{x}.{i}."
        n1, n2 = (f"norm1_{x}", f"norm2_{x}") if shared else ("norm1", "norm2")
        names += [pre + n1 + ".weight", pre + n1 + ".bias"] + [pre + k for k in BLOCK[:4]]
        names += [pre + n2 + ".weight", pre + n2 + ".bias"] + [pre + k for k in BLOCK[4:]]
    return names + [f"norm_{x}.weight", f"norm_{x}.bias"]


def classifier_keys(depth: int = 12) -> List[str]:
    """CAVClassifier.state_dict() restricted to what its forward touches: fusion_module, mae_a, mae_v (basic_model.py:93-107)."""
    return (["fusion_module.fc_out.weight", "fusion_module.fc_out.bias"] + ["mae_a." + k for k in branch_param_names("a", depth)]
            + ["mae_v." + k for k in branch_param_names("v", depth)])


def make_visual_params(seed: int, depth: int = 12, emb: int = 768, tokens: int = 196) -> Dict[str, torch.Tensor]:
    """Seeded visual-branch parameters, drawn like O.make_cavmae_audio_params draws the audio ones."""
    p: Dict[str, torch.Tensor] = {}
    for si, name in enumerate(branch_param_names("v", depth)):
        if name == "patch_embed_v.proj.weight":
            shp, std = (emb, 3, 16, 16), (2.0 / (emb + 768)) ** 0.5
        elif name == "pos_embed_v":
            shp, std = (1, tokens, emb), 0.5
        elif name == "modality_v":
            shp, std = (1, 1, emb), 0.02
        elif name.endswith("qkv.weight"):
            shp, std = (3 * emb, emb), (2.0 / (4 * emb)) ** 0.5
        elif name.endswith("qkv.bias"):
            shp, std = (3 * emb,), 0.02
        elif name.endswith("fc1.weight"):
            shp, std = (4 * emb, emb), (2.0 / (5 * emb)) ** 0.5
        elif name.endswith("fc1.bias"):
            shp, std = (4 * emb,), 0.02
        elif name.endswith("fc2.weight"):
            shp, std = (emb, 4 * emb), (2.0 / (5 * emb)) ** 0.5
        elif name.endswith("proj.weight"):
            shp, std = (emb, emb), (1.0 / emb) ** 0.5
        else:
            shp, std = (emb,), 0.02
        mean = 1.0 if ("norm" in name and name.endswith("weight")) else 0.0
        p[name] = O.portable_normal(seed, shp, stream=5000 + si, mean=mean, std=0.05 if mean else std)
    return p


def block(p, pre: str, n1: str, n2: str, x: torch.Tensor, heads: int, linear=F.linear) -> torch.Tensor:
    """cav_mae.py:103-113 with timm 0.4.5's Attention / Mlp; DropPath(0) is the identity."""
    B, n, D = x.shape
    h = F.layer_norm(x, (D,), p[pre + n1 + ".weight"], p[pre + n1 + ".bias"])
    qkv = linear(h, p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"]).reshape(B, n, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    att = F.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * (D // heads) ** -0.5, dim=-1)
    o = (att @ qkv[2]).transpose(1, 2).reshape(B, n, D)
    x = x + linear(o, p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"])
    h = F.layer_norm(x, (D,), p[pre + n2 + ".weight"], p[pre + n2 + ".bias"])
    h = F.gelu(linear(h, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"]))
    return x + linear(h, p[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"])


def visual_embed(p, image: torch.Tensor, linear=None) -> torch.Tensor:
    """patch_embed_v + pos_embed_v + modality_v (cav_mae.py:82, 353-355).  `linear`: the patch convolution as a Linear over
    (c, p1, p2)-flattened patches, for arithmetics that round the operands of every contraction."""
    if linear is None:
        v = F.conv2d(image, p["patch_embed_v.proj.weight"], p["patch_embed_v.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    else:
        v = linear(O.patchify(image), p["patch_embed_v.proj.weight"].flatten(1), p["patch_embed_v.proj.bias"])
    return v + p["pos_embed_v"] + p["modality_v"]


def visual_feature(p, image: torch.Tensor, heads: int = 12, linear=None) -> torch.Tensor:
    """CAVMAEFT.forward_feat(None, image, 'v') (cav_mae.py:352-364) + .mean(dim=1) (basic_model.py:123)."""
    x = visual_embed(p, image, linear)
    lin = F.linear if linear is None else linear
    depth = sum(1 for k in p if k.endswith("attn.qkv.weight"))
    for i in range(depth):
        if i < depth - 1:
            x = block(p, f"blocks_v.{i}.", "norm1", "norm2", x, heads, lin)                 # :357-358
        else:
            x = block(p, f"blocks_u.{i - (depth - 1)}.", "norm1_v", "norm2_v", x, heads, lin)   # :360-361
    return F.layer_norm(x, (x.shape[-1],), p["norm_v.weight"], p["norm_v.bias"]).mean(dim=1)


def cav_group_names(names: List[str]):
    """main.py:739-741 on `model.module.named_parameters()` names: (base group, mlp group).  The list names
    'module.fusion_module.fc_out.bias', which no name equals, so the head's bias stays in the base group."""
    mlp_list = ["fusion_module.fc_out.weight", "module.fusion_module.fc_out.bias"]
    return [n for n in names if n not in mlp_list], [n for n in names if n in mlp_list]


class CavState:
    """Parameters of the restated CAVClassifier as leaf tensors under the classifier's key names, and the optimiser of
    main.py:736-749 over them: Adam with the two --cav_opti groups, or SGD(momentum 0.9, weight decay 1e-4)."""

    def __init__(self, audio_p, visual_p, head, lr: float, optimizer: str = "adam"):
        self.p = {"fusion_module.fc_out.weight": head["weight"].clone(), "fusion_module.fc_out.bias": head["bias"].clone()}
        self.p.update({"mae_a." + k: v.clone() for k, v in audio_p.items()})
        self.p.update({"mae_v." + k: v.clone() for k, v in visual_p.items()})
        for v in self.p.values():
            v.requires_grad_(True)
        base, mlp = cav_group_names(list(self.p))
        if optimizer == "adam":
            self.opt = torch.optim.Adam([{"params": [self.p[n] for n in base], "lr": lr / 10}, {"params": [self.p[n] for n in mlp], "lr": lr}],
                                        weight_decay=5e-7, betas=(0.95, 0.999))
        else:
            self.opt = torch.optim.SGD(list(self.p.values()), lr=lr, momentum=0.9, weight_decay=1e-4)
        self.Pl = torch.eye(head["weight"].shape[1])
        self.exp_count = 0

    def branch(self, prefix: str):
        return {k[len(prefix):]: v for k, v in self.p.items() if k.startswith(prefix)}


def mla_iteration(st: CavState, spec, image, label, batch_index: int, len_dataloader: int, gs_mode: str = "as_intended") -> dict:
    """main.py:419-476 for args.lorb == 'large': joint forward, then per modality the shared head, CE, backward, GSPlugin
    on the head gradient (utils/utils.py:30-41 through O.gs_before_update), optimizer.step(), optimizer.zero_grad()."""
    out: dict = {}
    st.opt.zero_grad()                                                                     # main.py:164
    feats = {"a": O.cavmae_audio_feature(st.branch("mae_a."), spec), "v": visual_feature(st.branch("mae_v."), image)}   # :420
    W, b = st.p["fusion_module.fc_out.weight"], st.p["fusion_module.fc_out.bias"]
    for name in ("a", "v"):
        logits = F.linear(feats[name], W, b)                                               # :432 / :444 (the head already updated, Q7)
        loss = F.cross_entropy(logits, label)
        loss.backward()
        out["feat_" + name], out["out_" + name], out["loss_" + name] = feats[name].detach().clone(), logits.detach().clone(), loss.detach()
        out[f"head_grad_{name}_raw"] = W.grad.clone()
        st.Pl, W.grad = O.gs_before_update(st.Pl, feats[name].detach(), W.grad, batch_index, len_dataloader, st.exp_count, gs_mode)
        out[f"head_grad_{name}"] = W.grad.clone()
        out["grads_" + name] = {k: v.grad.clone() for k, v in st.p.items() if k.startswith(f"mae_{name}.") and v.grad is not None}
        st.opt.step()
        st.opt.zero_grad()
        st.exp_count += 1
    out["loss"] = out["loss_a"] * 0.55 + out["loss_v"] * 0.45                              # main.py:472 (Q8)
    return out
