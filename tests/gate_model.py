"""The numpy restatement of the gated fusion family w_m ~ a_m exp(-beta H_m) (include/mla_hip.h, mla_gate_sweep and
mla_eval_head_gated), row by row; fp64 by default, fp32 on request (for the conditions that only exist in fp32: the overflow caps).

Per batch row, E the eligible modalities: H_k = eval_model.row_entropy, hmax = max over E, and for a gate (a, beta)
x_k = beta (hmax - H_k), g_k = a_k exp(x_k) over E (+0.0 elsewhere), s = sum_k g_k (added in fp64, then cast), the pair is left out
unless s > 0, w_k = g_k / s, fused = sum_m w_m l_m in order, prediction = the first maximum.  The counting and the left-out policy
are sweep_model's."""
from types import SimpleNamespace

import numpy as np

import eval_model as EM
import sweep_model as SM

F32, F64 = np.float32, np.float64
LEFT_OUT = SM.LEFT_OUT
DENSE_SHAPES = [(2, 32, 6), (3, 65, 101), (3, 130, 128), (2, 5, 65)]          # (M, B, C), eval_model.sample_dense_case
DENSE_BETAS = (0, .25, .5, 1, 2, 4, 8, 16)
UNCOMPARED_CAP = 0.01               # the share of (row, gate) pairs a dense comparison may leave out as near ties


def entropies(outs, dtype=F64):
    """(B, M): H of every row and modality."""
    outs = np.asarray(outs, dtype=dtype)
    M, B, _ = outs.shape
    return np.array([[EM.row_entropy(outs[m][r], dtype) for m in range(M)] for r in range(B)], dtype=dtype).reshape(B, M)


def row_weights(logits, prior, beta, eligible, dtype=F64):
    """(w (M,), ok) of one row under one gate, operation by operation."""
    M = len(logits)
    el = np.asarray(eligible, dtype=bool)
    H = np.array([EM.row_entropy(l, dtype) for l in logits], dtype=dtype)
    hmax = dtype(-np.inf)
    for k in range(M):
        if el[k]:
            hmax = max(hmax, H[k])
    g = np.zeros(M, dtype=dtype)
    total = F64(0)
    for k in range(M):
        if el[k]:
            x = dtype(beta) * (hmax - H[k])
            g[k] = dtype(prior[k]) * np.exp(x)
        total = total + F64(g[k])
    s = dtype(total)
    w = np.zeros(M, dtype=dtype)
    if not s > 0:
        return w, False
    for k in range(M):
        if el[k]:
            w[k] = g[k] / s
    return w, True


def pairs(outs, labels, grid, present=None, dtype=F64):
    """Every (gate, row) pair at once: w (G, B, M), ok (G, B) (s > 0), fused (G, B, C), pred (G, B) int64 (LEFT_OUT where the pair is
    left out or the row is counted nowhere), margin (G, B): the top-two gap of the fused row, H (B, M)."""
    outs = np.asarray(outs, dtype=dtype)
    M, B, C = outs.shape
    grid = np.asarray(grid, dtype=dtype)
    a, beta = grid[:, :M], grid[:, M]
    el = np.ones((B, M), dtype=bool) if present is None else np.asarray(present).astype(bool)
    H = entropies(outs, dtype)
    hmax = np.where(el, H, -np.inf).max(axis=1)
    hmax = np.where(el.any(axis=1), hmax, 0).astype(dtype)                   # a row with nothing: counted nowhere, keep inf out
    x = beta[:, None, None] * (hmax[None, :, None] - H[None])
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(el[None], a[:, None, :] * np.exp(np.where(el[None], x, 0)), dtype(0)).astype(dtype)
        total = np.zeros(g.shape[:2], dtype=F64)
        for k in range(M):
            total = total + g[:, :, k].astype(F64)
        s = total.astype(dtype)
        ok = s > 0
        w = np.where(el[None] & ok[:, :, None], g / np.where(ok, s, 1)[:, :, None], dtype(0)).astype(dtype)
    fused = np.zeros((grid.shape[0], B, C), dtype=dtype)
    for m in range(M):
        fused = fused + w[:, :, m, None] * outs[m][None]
    counted = SM.row_counted(labels, C, present)
    pred = np.where(ok & counted[None], SM.first_max(fused), LEFT_OUT)
    top = np.sort(fused, axis=2)
    margin = top[:, :, -1] - top[:, :, -2] if C > 1 else np.full(fused.shape[:2], np.inf)
    return SimpleNamespace(w=w, ok=ok, fused=fused, pred=pred, margin=margin, H=H)


def sweep(outs, labels, grid, present=None, dtype=F64):
    """The three tables of one call: sweep_model's counting of this model's predictions."""
    C = np.asarray(outs).shape[2]
    return SM.count_tables(pairs(outs, labels, grid, present, dtype).pred, labels, C, present)


def margin_floor(M, grid, outs):
    """(G,): the fp64 top-two margin below which a pair is not compared: M (1 + beta) WEIGHT_TOL max|logit| -- the project's weight
    tolerance carried through the fused sum, scaled by 1 + beta because an entropy error d moves g_k by the factor e^(beta d)."""
    beta = np.asarray(grid, dtype=F64)[:, M]
    return M * (1 + beta) * EM.WEIGHT_TOL * max(float(np.abs(o).max()) for o in outs)


def dense_grid(M):
    from mla_hip import gate_grid
    return gate_grid(M, betas=DENSE_BETAS, steps=20 if M == 2 else 8).numpy()


_DENSE = {}


def dense_case(M, B, C):
    """(outs (M, B, C) fp32, labels, grid, fp64 model, compared (G, B) bool) of one dense shape, formed once and shared."""
    if (M, B, C) not in _DENSE:
        outs, labels = EM.sample_dense_case(M, B, C)
        outs = np.stack(outs).astype(F32)
        grid = dense_grid(M)
        model = pairs(outs, labels, grid)
        compared = model.ok & (model.margin >= margin_floor(M, grid, outs)[:, None])
        for v in (compared, model.pred, model.w, model.fused):
            v.setflags(write=False)
        _DENSE[(M, B, C)] = (outs, labels, grid, model, compared)
    return _DENSE[(M, B, C)]
