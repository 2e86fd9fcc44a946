"""CPU restatement of the reference's `--clip` model for the tests (models/basic_model.py:278-319, main.py:428-454, 273-311, 416).

  clip_forward   CLIPClassifier.forward: squeeze dim 1; gs_flag: (token, visual), else (a, v, fc_out(cat(a, v)))
  ClipState      what the gs step mutates: the head, its SGD momentum, Pl, exp_count
  gs_phase       one modality phase (main.py:432-442) composed of the oracle's head_ce_fwd_bwd, gs_before_update and sgd_step
  clip_gs_step   the two phases of main.py:428-454 and the reported loss (:472)
  joint_step     the gs_flag-false step (main.py:164, 273-311, 416) in plain torch autograd with torch.optim.SGD

Everything takes the dtype of what it is handed (fp32 state: the fp32 oracle; fp64 state: the same phase in double).
tests/golden/make_golden_clip.py asserts that this agrees with the reference's own modules.
"""
import torch

from oracle import mla_oracle as O


def clip_forward(token, visual, gs_flag, W=None, b=None):
    a, v = token.squeeze(1), visual.squeeze(1)                                   # basic_model.py:314-315
    if gs_flag:
        return a, v                                                              # :319
    return a, v, torch.cat((a, v), dim=1) @ W.t() + b                            # :317, fusion_modules.py:22-23


class ClipState:
    def __init__(self, head, d=512):
        self.head = {k: v.clone() for k, v in head.items()}
        self.mom = {"weight": None, "bias": None}
        self.Pl = torch.eye(d, dtype=head["weight"].dtype)
        self.exp_count = 0

    def clone(self, dtype=None):
        s = ClipState.__new__(ClipState)
        cv = (lambda t: t.clone()) if dtype is None else (lambda t: t.to(dtype))
        s.head = {k: cv(v) for k, v in self.head.items()}
        s.mom = {k: None if v is None else cv(v) for k, v in self.mom.items()}
        s.Pl, s.exp_count = cv(self.Pl), self.exp_count
        return s


def gs_phase(st, X, label, batch_index, len_dataloader, lr=1e-3, momentum=0.9, wd=1e-4, gs_mode="as_intended"):
    """main.py:432-442 on the state, in place.  Returns logits, loss, the raw and the projected weight gradient, the bias gradient."""
    W, b = st.head["weight"], st.head["bias"]
    logits, loss, dW, db, _dX = O.head_ce_fwd_bwd(X, W, b, label)                # :432-435
    raw = dW.clone()
    st.Pl, dW = O.gs_before_update(st.Pl, X, dW, batch_index, len_dataloader, st.exp_count, gs_mode)      # :437
    st.head["weight"], st.mom["weight"] = O.sgd_step(W, dW, st.mom["weight"], lr, momentum, wd)           # :439
    st.head["bias"], st.mom["bias"] = O.sgd_step(b, db, st.mom["bias"], lr, momentum, wd)
    st.exp_count += 1                                                            # :442
    return {"out": logits, "loss": loss, "grad_raw": raw, "grad": dW, "bias_grad": db}


def clip_gs_step(st, token, visual, label, batch_index, len_dataloader, lr=1e-3, momentum=0.9, wd=1e-4, gs_mode="as_intended",
                 av_alpha=0.55):
    a, v = clip_forward(token, visual, True)                                     # main.py:428-429
    pa = gs_phase(st, a, label, batch_index, len_dataloader, lr, momentum, wd, gs_mode)
    pv = gs_phase(st, v, label, batch_index, len_dataloader, lr, momentum, wd, gs_mode)      # the head the token phase updated (Q7)
    return {"a": a, "v": v, "out_a": pa["out"], "out_v": pv["out"], "loss_a": pa["loss"], "loss_v": pv["loss"],
            "loss": pa["loss"] * av_alpha + pv["loss"] * (1 - av_alpha),         # :472 (Q8)
            "head_grad_a": pa["grad"], "head_grad_v": pv["grad"]}


class JointRef:
    """The gs_flag-false step in plain torch autograd: fc_out = Linear(2 D, C) on cat(token, visual), torch.optim.SGD."""

    def __init__(self, head, lr=1e-3, momentum=0.9, wd=1e-4):
        self.W = head["weight"].clone().requires_grad_(True)
        self.b = head["bias"].clone().requires_grad_(True)
        self.opt = torch.optim.SGD([self.W, self.b], lr=lr, momentum=momentum, weight_decay=wd)           # main.py:749

    def step(self, token, visual, label):
        crit = torch.nn.CrossEntropyLoss()
        self.opt.zero_grad()                                                     # main.py:164
        a, v, out = clip_forward(token, visual, False, self.W, self.b)           # :273
        D = self.W.shape[1] // 2
        out_v = v @ self.W[:, D:].t() + self.b / 2                               # :298-299
        out_a = a @ self.W[:, :D].t() + self.b / 2                               # :301-302
        loss, loss_a, loss_v = crit(out, label), crit(out_a, label), crit(out_v, label)                   # :305-309
        loss.backward()                                                          # :310
        rec = {"out": out.detach().clone(), "out_a": out_a.detach().clone(), "out_v": out_v.detach().clone(),
               "loss": loss.detach().clone(), "loss_a": loss_a.detach().clone(), "loss_v": loss_v.detach().clone()}
        self.opt.step()                                                          # :416
        rec["weight"], rec["bias"] = self.W.detach().clone(), self.b.detach().clone()
        return rec


def clip_inputs(seed, step, B, D, C, absolute=True):
    """Stored-feature stand-ins from the portable generator: mean 0.3, std 0.7 (the regime of gs_kat_d512), `.abs()` unless the
    mixed-sign case is wanted.  Shapes as the loader yields them: (B, 1, D)."""
    tok = O.portable_normal(seed + step, (B, 1, D), stream=21, mean=0.3, std=0.7)
    img = O.portable_normal(seed + step, (B, 1, D), stream=22, mean=0.3, std=0.7)
    if absolute:
        tok, img = tok.abs(), img.abs()
    return tok, img, O.portable_labels(seed + step, B, C)
