"""FusedSGD / FusedAdam: torch.optim.SGD(momentum, weight_decay) (main.py:749) and torch.optim.Adam (main.py:736-747, --cav_opti)
semantics over flat buffers.  What follows is written for FusedSGD; FusedAdam shares all of it (`FlatOptimizer`) except the
launch and the state it keeps (see its docstring).

Two ways in, one engine (one `mla_sgd_step` launch per flat buffer = per encoder / head):

  * protocol mode -- `FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)`, the drop-in for
    `optim.SGD(...)` at main.py:749.  It is a real `torch.optim.Optimizer` (param_groups, `StepLR` at main.py:760 works,
    torch-format `state_dict()` with per-parameter `momentum_buffer`s in reference layout), but the parameters it
    receives are views of flat buffers (module.py): `step()` finds each parameter's owner and launches once per owner.
    Semantics per owner, exactly torch's per-parameter rule: all `.grad` None -> skipped (torch >= 2 after
    `zero_grad()`), gradients present -> weight decay + momentum + update; `zero_grad(set_to_none=False)` reproduces
    pinned torch 1.8.1, where zeroed gradients still receive weight decay + momentum.  Gradients somebody
    else assigned (not the published flat views) are copied into the flat gradient first; a partially-None owner
    falls back to one launch per parameter segment.
  * trainer mode -- `FusedSGD({"audio": enc_a, "visual": enc_v, "head": head}, ...)`: MLATrainer drives the groups
    explicitly (`mark_ready` / `step_group`) on their own streams.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Union

import torch

from . import ops
from ._lib import MLAHipError


class FlatOptimizer(torch.optim.Optimizer):
    """What FusedSGD and FusedAdam share: owner discovery (protocol mode) / named owners (trainer mode), torch's per-parameter
    skip rule applied per owner in `step()` with the foreign / partial gradient handling, `zero_grad`, and the trainer-mode
    `none` / `zero` / `ready` state machine.  A subclass keeps its state and supplies `_launch(name, with_grad)` (one owner, all
    of it) and `_launch_segments(name, has_grad)` (per registered parameter; has_grad[i] None = skip that one)."""

    def __init__(self, params: Union[Dict[str, object], Iterable], defaults: dict, legacy_zero_grad: bool = False,
                 param_groups: Optional[list] = None):
        """param_groups (trainer mode only): torch-style groups over the owners' parameters instead of one group of all."""
        self.legacy_zero_grad = legacy_zero_grad
        if isinstance(params, dict):                          # trainer mode: name -> object with .flat / .grad
            self.groups = dict(params)
            plist = [p for g in self.groups.values() for p in self._owner_params(g)]
            self.protocol = False
            if param_groups is not None:
                plist = list(param_groups)
        else:
            plist = list(params)
            owners: List[object] = []
            for p in plist:
                for q in (p["params"] if isinstance(p, dict) else [p]):
                    owner = getattr(q, "_mla_owner", None)
                    if owner is None:
                        raise MLAHipError("%s drives mla_hip parameters only (views of the kernels' flat buffers); "
                                          "got a foreign tensor of shape %s" % (type(self).__name__, tuple(q.shape)))
                    if not any(o is owner for o in owners):
                        owners.append(owner)
            self.groups = {"%s%d" % (type(o).__name__, i): o for i, o in enumerate(owners)}
            self.protocol = True
        if not plist:       # trainer-mode stand-ins without registered parameters (host-logic tests)
            plist = [torch.zeros(1, requires_grad=True)]
        super().__init__(plist, defaults)
        # trainer mode: gradient state per group: "none" | "zero" | "ready"
        self.grad_state = {k: "none" for k in self.groups}

    @staticmethod
    def _owner_params(g) -> list:
        return [p for _n, p, _gv in getattr(g, "_entries", [])]

    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    def set_lr(self, lr: float) -> None:
        for grp in self.param_groups:
            grp["lr"] = lr

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self.protocol:                                       # trainer mode
            for k in self.groups:
                self.step_group(k)
            return loss
        for name, g in self.groups.items():                         # protocol mode: torch's per-parameter rule, per owner
            works = getattr(g, "_grad_works", None)
            if works:
                g.comm.wait(works)                                  # data parallel: encoder gradients reduced
                g._grad_works = []
            state = g.grads_alias_flat()
            if state is None:
                continue                                            # every p.grad is None -> skipped (torch >= 2 zero_grad)
            if state:
                self._launch(name, True)
                continue
            has = []
            for i, (_n, p, gv) in enumerate(g._entries):            # foreign or partial gradients
                if p.grad is None:
                    has.append(None)
                    continue
                if g._published is None or p.grad is not g._published[i]:
                    gv.copy_(p.grad)
                    p.grad = gv
                has.append(True)
            if g._published is None:
                g._published = [None] * len(g._entries)
            for i, (_n, p, gv) in enumerate(g._entries):
                if has[i]:
                    g._published[i] = gv
            if all(h for h in has):
                self._launch(name, True)
            else:
                self._launch_segments(name, has)
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """main.py:164, 440, 452.  set_to_none=False (or legacy_zero_grad) = torch 1.8.1: tensors stay, zero-filled."""
        if not self.protocol:
            for k in self.groups:
                if self.grad_state[k] != "none":
                    self.grad_state[k] = "zero" if self.legacy_zero_grad else "none"
            return
        if set_to_none and not self.legacy_zero_grad:
            for g in self.groups.values():
                for _n, p, _gv in g._entries:
                    p.grad = None
            return
        for g in self.groups.values():
            state = g.grads_alias_flat()
            if state is None:
                continue
            if state:
                g.grad.zero_()                                      # one memset for the whole owner
            else:
                for _n, p, _gv in g._entries:
                    if p.grad is not None:
                        p.grad.zero_()

    # ---- trainer-mode state machine ---------------------------------------------------------------------------------
    def mark_ready(self, name: str) -> None:
        self.grad_state[name] = "ready"

    def step_group(self, name: str) -> None:
        state = self.grad_state[name]
        if state == "none":
            return                                                  # p.grad is None -> skipped by torch.optim.SGD / Adam
        self._launch(name, state == "ready")                        # "zero": zeroed grads (1.8.1): wd + momentum still apply

    def drop_grads(self) -> None:
        """main.py:468-470: `del p.grad` for every parameter."""
        for k in self.groups:
            self.grad_state[k] = "none"

    def _state_view(self, buf: torch.Tensor, name: str, i: int) -> torch.Tensor:
        """Reference-layout view of parameter i's range of a per-owner state buffer laid out like the owner's flat buffers."""
        g = self.groups[name]
        gv = g._entries[i][2]
        return torch.as_strided(buf, gv.shape, gv.stride(), gv.storage_offset() - g.grad.storage_offset())


class FusedSGD(FlatOptimizer):
    def __init__(self, params: Union[Dict[str, object], Iterable], lr: float = 1e-3, momentum: float = 0.9,
                 weight_decay: float = 1e-4, legacy_zero_grad: bool = False):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay), legacy_zero_grad)
        self.buf = {k: torch.zeros_like(g.flat) for k, g in self.groups.items()}
        self.initialized = {k: False for k in self.groups}
        self.seg_initialized: Dict[str, Optional[List[bool]]] = {k: None for k in self.groups}   # only after a partial step

    # ---- hyper-parameters live in param_groups (so lr schedulers work) ---------------------------------------
    def _hyper(self, name: str):
        owner = self.groups[name]
        first = self._owner_params(owner)
        for grp in self.param_groups:
            if not first or any(q is first[0] for q in grp["params"]):
                return grp["lr"], grp["momentum"], grp["weight_decay"]
        g0 = self.param_groups[0]
        return g0["lr"], g0["momentum"], g0["weight_decay"]

    # ---- engine -------------------------------------------------------------------------------------------------
    def _launch(self, name: str, with_grad: bool) -> None:
        g = self.groups[name]
        lr, mom, wd = self._hyper(name)
        if self.seg_initialized[name] is not None:
            self._launch_segments(name, [with_grad] * len(g._entries))
            return
        ops.sgd_step(g.flat, g.grad if with_grad else None, self.buf[name], lr, mom, wd, first=not self.initialized[name])
        self.initialized[name] = True

    def _launch_segments(self, name: str, has_grad: List[Optional[bool]]) -> None:
        """Per-parameter launches (only when an owner's gradients are partially None): has_grad[i] None = skip."""
        g = self.groups[name]
        lr, mom, wd = self._hyper(name)
        if self.seg_initialized[name] is None:
            self.seg_initialized[name] = [self.initialized[name]] * len(g._entries)
        seg = self.seg_initialized[name]
        for i, (o, n) in enumerate(g.segments()):
            if has_grad[i] is None:
                continue
            ops.sgd_step(g.flat[o:o + n], g.grad[o:o + n] if has_grad[i] else None, self.buf[name][o:o + n], lr, mom, wd,
                         first=not seg[i])
            seg[i] = True
        self.initialized[name] = self.initialized[name] or all(seg)

    # ---- (de)serialisation: torch's format, momentum buffers in reference layout -------------------------------------
    def _mom_view(self, name: str, i: int) -> torch.Tensor:
        return self._state_view(self.buf[name], name, i)

    def state_dict(self) -> dict:
        """torch.optim.SGD's layout (main.py:922): {'state': {index: {'momentum_buffer': tensor}}, 'param_groups': [...]}
        with parameters indexed in `model.parameters()` order; buffers are contiguous copies in the reference layout."""
        for name, g in self.groups.items():
            g._await_tail()
            seg = self.seg_initialized[name]
            for i, (_n, p, _gv) in enumerate(getattr(g, "_entries", [])):
                if (seg[i] if seg is not None else self.initialized[name]):
                    self.state[p]["momentum_buffer"] = self._mom_view(name, i).clone(memory_format=torch.contiguous_format)
                else:
                    self.state.pop(p, None)
        sd = super().state_dict()
        sd["mla_hip"] = {"initialized": dict(self.initialized)}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Accepts a torch.optim.SGD state_dict of the reference (same parameter order) or one of our own."""
        sd = dict(sd)
        sd.pop("mla_hip", None)
        super().load_state_dict(sd)
        for name, g in self.groups.items():
            ents = getattr(g, "_entries", [])
            seg = []
            for i, (_n, p, _gv) in enumerate(ents):
                mb = self.state.get(p, {}).get("momentum_buffer")
                seg.append(mb is not None)
                if mb is not None:
                    self._mom_view(name, i).copy_(mb)
            self.initialized[name] = bool(seg) and all(seg)
            self.seg_initialized[name] = None if (all(seg) or not any(seg)) else seg


class FusedAdam(FlatOptimizer):
    """torch.optim.Adam (amsgrad=False, maximize=False; main.py:736-747 `--cav_opti`, main.py:31) with FusedSGD's two entrances.

    State per owner: flat `m` / `v` beside the owner's flat buffers and a step counter.  The counter advances only when the owner
    is actually stepped (all `.grad` None / trainer state "none": skipped, no advance -- torch counts per parameter), so in the MLA
    loop the head counts two steps per iteration and each encoder one; after a partial step it is kept per parameter.
    Hyper-parameters are read per parameter from its `param_group` at every launch (MultiStepLR / StepLR just work).  Ranges that
    lie next to each other in the flat buffer and agree in hyper-parameters, step count and gradient state take ONE
    `mla_adam_step` launch: an owner with uniform hyper-parameters is one launch, the `cav_param_groups` head (weight at lr, bias
    at lr/10) is two.

    Trainer mode: `FusedAdam({"audio": enc, ..., "head": head}, lr=...)`; `lr` may be a mapping owner name -> lr (one group per
    owner), or `param_groups=` torch-style groups over the owners' parameters (e.g. `cav_param_groups(model, lr)`)."""

    def __init__(self, params: Union[Dict[str, object], Iterable], lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, legacy_zero_grad: bool = False, param_groups: Optional[list] = None):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        if isinstance(lr, dict):
            if not isinstance(params, dict) or param_groups is not None:
                raise MLAHipError("FusedAdam: a per-owner lr mapping needs the trainer-mode owner dict (and no param_groups)")
            missing = [k for k in params if k not in lr]
            if missing:
                raise MLAHipError(f"FusedAdam: the lr mapping lacks the owners {missing}")
            param_groups = [{"params": self._owner_params(o), "lr": lr[k]} for k, o in params.items() if self._owner_params(o)]
            defaults["lr"] = next(iter(lr.values()))
        super().__init__(params, defaults, legacy_zero_grad, param_groups or None)
        self.m = {k: torch.zeros_like(g.flat) for k, g in self.groups.items()}
        self.v = {k: torch.zeros_like(g.flat) for k, g in self.groups.items()}
        self.steps = {k: 0 for k in self.groups}
        self.seg_steps: Dict[str, Optional[List[int]]] = {k: None for k in self.groups}     # only after a partial step

    def _group_of(self, p) -> dict:
        """The param_group that holds p (looked up per launch: schedulers rewrite the groups' values in place)."""
        for grp in self.param_groups:
            if any(q is p for q in grp["params"]):
                return grp
        return self.param_groups[0]

    def _hypers(self, name: str) -> list:
        """(lr, beta1, beta2, eps, weight_decay) of every registered parameter of the owner (one entry for a stand-in)."""
        hy = lambda grp: (grp["lr"], grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"])
        ents = self._owner_params(self.groups[name])
        return [hy(self._group_of(p)) for p in ents] if ents else [hy(self.param_groups[0])]

    # ---- engine -------------------------------------------------------------------------------------------------
    def _check_single_process(self, g) -> None:
        comm = getattr(g, "comm", None)
        if comm is not None and getattr(comm, "world", 1) > 1:
            raise MLAHipError("FusedAdam is not implemented for data-parallel training (comm.world > 1)")

    def _launch(self, name: str, with_grad: bool) -> None:
        g = self.groups[name]
        hy = self._hypers(name)
        if self.seg_steps[name] is not None or len(set(hy)) > 1:
            self._launch_segments(name, [with_grad] * len(g._entries), hy)
            return
        self._check_single_process(g)
        self.steps[name] += 1
        ops.adam_step(g.flat, g.grad if with_grad else None, self.m[name], self.v[name], *hy[0], self.steps[name])

    def _launch_segments(self, name: str, has_grad: List[Optional[bool]], hy: Optional[list] = None) -> None:
        """Launches over runs of parameters (partially-None gradients, or more than one param_group in the owner)."""
        g = self.groups[name]
        self._check_single_process(g)
        hy = hy or self._hypers(name)
        partial = any(h is None for h in has_grad)
        seg = self.seg_steps[name]
        if seg is None and partial:
            seg = self.seg_steps[name] = [self.steps[name]] * len(g._entries)
        if seg is None:
            self.steps[name] += 1
        runs: list = []                                    # [offset, numel, with_grad, hyper, step]
        for i, (o, n) in enumerate(g.segments()):
            if has_grad[i] is None:
                continue
            if seg is not None:
                seg[i] += 1
            key = (bool(has_grad[i]), hy[i], seg[i] if seg is not None else self.steps[name])
            if runs and runs[-1][2:] == list(key) and runs[-1][0] + runs[-1][1] == o:
                runs[-1][1] += n
            else:
                runs.append([o, n, *key])
        for o, n, wg, h, step in runs:
            ops.adam_step(g.flat[o:o + n], g.grad[o:o + n] if wg else None, self.m[name][o:o + n], self.v[name][o:o + n], *h, step)
        if seg is not None:
            self.steps[name] = max(seg)
            if len(set(seg)) == 1:                         # every parameter caught up: back to one counter
                self.seg_steps[name] = None

    # ---- (de)serialisation: torch.optim.Adam's format, moments in reference layout -----------------------------------
    def state_dict(self) -> dict:
        """{'state': {index: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]}, parameters indexed in the order they were
        given (`model.parameters()`); moments are contiguous copies in the reference layout, `step` a float32 scalar tensor as
        torch.optim.Adam keeps it.  Loads into torch.optim.Adam over the same parameters."""
        for name, g in self.groups.items():
            if hasattr(g, "_await_tail"):
                g._await_tail()
            seg = self.seg_steps[name]
            for i, (_n, p, _gv) in enumerate(getattr(g, "_entries", [])):
                step = seg[i] if seg is not None else self.steps[name]
                if step > 0:
                    self.state[p] = {"step": torch.tensor(float(step)),
                                     "exp_avg": self._state_view(self.m[name], name, i).clone(memory_format=torch.contiguous_format),
                                     "exp_avg_sq": self._state_view(self.v[name], name, i).clone(memory_format=torch.contiguous_format)}
                else:
                    self.state.pop(p, None)
        return super().state_dict()

    def load_state_dict(self, sd: dict) -> None:
        """Accepts a torch.optim.Adam state_dict over the same parameters (same order) or one of our own."""
        super().load_state_dict(sd)
        for name, g in self.groups.items():
            seg = []
            for i, (_n, p, _gv) in enumerate(getattr(g, "_entries", [])):
                st = self.state.get(p, {})
                seg.append(int(st["step"]) if "step" in st else 0)
                for key, buf in (("exp_avg", self.m), ("exp_avg_sq", self.v)):
                    view = self._state_view(buf[name], name, i)
                    view.copy_(st[key]) if key in st else view.zero_()
            self.steps[name] = max(seg) if seg else 0
            self.seg_steps[name] = None if len(set(seg)) <= 1 else seg


def cav_param_groups(model, lr: float) -> list:
    """The two parameter groups of the reference's `--cav_opti` optimiser (main.py:739-745), typo included: the names listed for
    the `lr` group are 'fusion_module.fc_out.weight' and 'module.fusion_module.fc_out.bias', matched against
    `model.module.named_parameters()`, whose names carry no 'module.' prefix.  So only fc_out.weight trains at `lr`; fc_out.bias
    falls into the base group with every encoder parameter, at lr / 10 -- [base group, head group], as the reference orders them."""
    head_names = ("fusion_module.fc_out.weight", "module.fusion_module.fc_out.bias")
    named = list(model.module.named_parameters())
    head = [p for n, p in named if n in head_names]
    base = [p for n, p in named if n not in head_names]
    return [{"params": base, "lr": lr / 10}, {"params": head, "lr": lr}]
