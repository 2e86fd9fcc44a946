"""The numpy restatement of mla_fusion_sweep (include/mla_hip.h): the fixed-weight fusion of one batch at every row of a grid of
fusion weights, in fp32, operation by operation.

  fused=False   every product and every sum is rounded to fp32 on its own: v = fl(v + fl(w * x))
  fused=True    every step is one fused multiply-add: v = float32(float64(v) + float64(w) * float64(x)).  The fp64 product of two
                fp32 numbers is exact; the fp64 sum rounds once more before the cast, which the near-tie inputs of
                tests/test_sweep_gpu.py are built to be untouched by

and the integer counting that turns predictions into the tp / pp / num tables.  On exactly-summable inputs (integer logits, weights
that are multiples of 2^-8) the two forms agree and the restatement is the definition, bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64
LEFT_OUT = -1            # predict(): the (grid row, batch row) pair adds nothing to tp or pp


def row_counted(labels, C, present=None):
    """(B,) bool: the rows that are counted at all -- a label inside [0, C) and a present modality."""
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels < C)
    if present is not None:
        ok &= np.asarray(present).astype(bool).any(axis=1)
    return ok


def pair_weights(grid, B, present=None):
    """(w (G, B, M) fp32, ok (G, B) bool): the weights of every (grid row, batch row) pair.  A row that has every modality uses
    grid[g] as it is; otherwise s = the eligible entries added in order from +0.0, w = eligible ? grid[g][m] / s : +0.0, and the
    pair is left out unless s > 0."""
    grid = np.asarray(grid, dtype=F32)
    G, M = grid.shape
    w = np.broadcast_to(grid[:, None, :], (G, B, M)).copy()
    ok = np.ones((G, B), dtype=bool)
    if present is None:
        return w, ok
    el = np.asarray(present).astype(bool)
    partial = ~el.all(axis=1)
    for r in np.flatnonzero(partial):
        s = np.zeros(G, dtype=F32)
        for m in range(M):
            if el[r, m]:
                s = s + grid[:, m]
        with np.errstate(divide="ignore", invalid="ignore"):
            for m in range(M):
                w[:, r, m] = grid[:, m] / s if el[r, m] else F32(0)
        ok[:, r] = s > 0
    return w, ok


def fuse(w, outs, fused=False):
    """(G, B, C) fp32: sum_m w_m l_m[c], modalities in order from +0.0."""
    outs = np.asarray(outs, dtype=F32)
    M, B, C = outs.shape
    v = np.zeros((w.shape[0], B, C), dtype=F32)
    for m in range(M):
        wm, x = w[:, :, m, None], outs[m][None]
        if fused:
            v = (v.astype(F64) + wm.astype(F64) * x.astype(F64)).astype(F32)
        else:
            v = v + wm * x
    return v


def first_max(v):
    """The first maximum along the last axis: the `v > best` scan from -inf with arg = 0 (numpy.argmax on finite rows)."""
    return np.argmax(v, axis=-1)


def predict(outs, labels, grid, present=None, fused=False, chunk=64):
    """(G, B) int64: the prediction of every pair, LEFT_OUT where the pair is left out or the row is counted nowhere."""
    outs = np.asarray(outs, dtype=F32)
    M, B, C = outs.shape
    grid = np.asarray(grid, dtype=F32)
    counted = row_counted(labels, C, present)
    pred = np.full((grid.shape[0], B), LEFT_OUT, dtype=np.int64)
    for g0 in range(0, grid.shape[0], chunk):
        w, ok = pair_weights(grid[g0:g0 + chunk], B, present)
        w[~ok] = 0                                           # left out below: keep NaN and inf out of the arithmetic
        p = first_max(fuse(w, outs, fused))
        pred[g0:g0 + chunk] = np.where(ok & counted[None], p, LEFT_OUT)
    return pred


def count_tables(pred, labels, C, present=None):
    """(tp (G, C), pp (G, C), num (C)) int64 from predictions (G, B): num once per counted row; pp[g][prediction] and, where it is
    the label, tp[g][label] for every pair that is not LEFT_OUT."""
    pred, labels = np.asarray(pred), np.asarray(labels)
    counted = row_counted(labels, C, present)
    num = np.bincount(labels[counted].astype(np.int64), minlength=C).astype(np.int64)
    G = pred.shape[0]
    tp, pp = np.zeros((G, C), dtype=np.int64), np.zeros((G, C), dtype=np.int64)
    for g in range(G):
        live = counted & (pred[g] != LEFT_OUT)
        pp[g] = np.bincount(pred[g][live], minlength=C)
        tp[g] = np.bincount(labels[live & (pred[g] == labels)].astype(np.int64), minlength=C)
    return tp, pp, num


def sweep(outs, labels, grid, present=None, fused=False):
    """The three tables of one call."""
    C = np.asarray(outs).shape[2]
    return count_tables(predict(outs, labels, grid, present, fused), labels, C, present)


def confusion_of(pred_g, labels, C, present=None):
    """(C, C) [true][predicted] of one grid row's predictions over the pairs that made one."""
    labels = np.asarray(labels)
    live = row_counted(labels, C, present) & (pred_g != LEFT_OUT)
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (labels[live].astype(np.int64), pred_g[live]), 1)
    return conf


def exact_case(M, B, C, G, seed):
    """Exactly-summable inputs: integer logits in [-512, 512] on a coarse lattice (many exact ties between classes), grid weights
    that are multiples of 2^-8 in [0, 1].  Every product and every partial sum is an fp32 number, so rounding and contraction
    cannot matter and only the first-maximum rule decides ties."""
    rng = np.random.default_rng(seed)
    outs = (rng.integers(-4, 5, size=(M, B, C)) * 128).astype(F32)
    outs[:, :, C // 2:] = outs[:, :, :C - C // 2][:, :, ::-1].copy()                         # mirrored halves: ties across the row
    grid = (rng.integers(0, 257, size=(G, M)) / 256).astype(F32)
    grid[0] = 0                                              # all fused values +0.0: the first class
    if G > 1:
        grid[1] = 0
        grid[1, 0] = 1                                       # modality 0 alone
    labels = rng.integers(0, C, size=B).astype(np.int64)
    return outs, labels, grid
