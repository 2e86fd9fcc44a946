"""CPU restatement of the QMF joint step for the tests (tests/test_qmf_cpu.py, tests/test_qmf_gpu.py): the formulas of
main.py:170-268 / 108-125 in fp64 torch autograd, the History of utils/utils.py:44-95 in numpy, and the rule numpy's buffered
`a[idx] += v` follows for an index that occurs more than once in a batch (the last occurrence writes).  Not product code."""
import numpy as np
import torch


class History:
    """utils/utils.py:44-95 for one modality."""

    def __init__(self, n_data):
        self.correctness = np.zeros(n_data)
        self.confidence = np.zeros(n_data)

    def update(self, idx, ell, conf):
        """correctness[idx] += ell; confidence[idx] = conf, written out with ONE writer per entry: of several samples that
        carry the same index only the last one counts (what numpy's fancy-index `+=` / `=` do)."""
        idx = np.asarray(idx).reshape(-1)
        ell, conf = np.asarray(ell, dtype=np.float64).reshape(-1), np.asarray(conf, dtype=np.float64).reshape(-1)
        for i in range(len(idx)):
            if idx[i] in idx[i + 1:]:
                continue
            self.correctness[idx[i]] += ell[i]
            self.confidence[idx[i]] = conf[i]

    def normalize(self, data):
        lo, hi = self.correctness.min(), self.correctness.max()
        with np.errstate(invalid="ignore", divide="ignore"):
            return (data - lo) / (hi - lo)

    def target_margin(self, idx):
        """(t, mg) of the pairs (i, (i + 1) mod B): t = sign(n_i - n_j), mg = |n_i - n_j| (fp64)."""
        idx = np.asarray(idx).reshape(-1)
        n1 = self.normalize(self.correctness[idx])
        n2 = self.normalize(self.correctness[np.roll(idx, -1)])
        t = (n1 > n2).astype(np.float64) - (n1 < n2).astype(np.float64)
        return t, np.abs(n1 - n2)


def rank_loss(conf, t, mg):
    """main.py:108-125 with target t and margin mg given: mean_i max(0, t_i (c_i - r_i)), r_i = c_j + mg_i / (t_i ? t_i : 1)."""
    t = torch.as_tensor(t, dtype=conf.dtype, device=conf.device)
    mg = torch.as_tensor(mg, dtype=conf.dtype, device=conf.device)
    r = torch.roll(conf, -1) + mg / torch.where(t == 0, torch.ones_like(t), t)
    return torch.clamp_min(t * (conf - r), 0).mean()


def qmf_step(xs, Ws, bs, label, idx, hists, w_cml, w_crl, dtype=torch.float64):
    """One QMF training step on features xs[m] (B, D) with heads (Ws[m], bs[m]); `hists[m]` (History) is updated.  Returns a dict of
    fp64 tensors: z (M, B, C), out, conf (M, B), ell (M, B), target, margin, rank (M), ce (M), cml, loss, dW / db / dX lists."""
    xs = [torch.as_tensor(x).detach().to(dtype).cpu().requires_grad_(True) for x in xs]
    Ws = [torch.as_tensor(W).detach().to(dtype).cpu().requires_grad_(True) for W in Ws]
    bs = [torch.as_tensor(b).detach().to(dtype).cpu().requires_grad_(True) for b in bs]
    label = torch.as_tensor(label).cpu().reshape(-1)
    idx = np.asarray(torch.as_tensor(idx).cpu()).reshape(-1)
    M, B = len(xs), xs[0].shape[0]
    z = [xs[m] @ Ws[m].T + bs[m] for m in range(M)]
    E = [torch.logsumexp(z[m], dim=1) for m in range(M)]
    conf = [E[m] / 10 for m in range(M)]
    out = sum(conf[m].detach().reshape(-1, 1) * z[m] for m in range(M))
    ell = [E[m] - z[m][torch.arange(B), label] for m in range(M)]
    ce = [ell[m].mean() for m in range(M)]
    ts, mgs, ranks = [], [], []
    for m in range(M):
        # the History stores what the fp32 reference hands it: fp32 losses and confidences
        hists[m].update(idx, ell[m].detach().float().numpy(), conf[m].detach().float().numpy())
        t, mg = hists[m].target_margin(idx)
        ts.append(t)
        mgs.append(mg)
        ranks.append(rank_loss(conf[m], t, np.float32(mg).astype(np.float64)))
    cml = (torch.logsumexp(out, dim=1) - out[torch.arange(B), label]).mean()
    loss = w_cml * cml + sum(ce) + w_crl * sum(ranks)
    loss.backward()
    return {"z": torch.stack([t_.detach() for t_ in z]), "out": out.detach(), "conf": torch.stack([c.detach() for c in conf]),
            "ell": torch.stack([e.detach() for e in ell]), "target": torch.from_numpy(np.stack(ts)),
            "margin": torch.from_numpy(np.stack(mgs)), "rank": torch.stack([r.detach() for r in ranks]),
            "ce": torch.stack([c.detach() for c in ce]), "cml": cml.detach(), "loss": loss.detach(),
            "dW": [W.grad for W in Ws], "db": [b.grad for b in bs], "dX": [x.grad for x in xs]}


def head_inputs(O, seed, M, B, D, C):
    """The head-level fixture cases' inputs, a pure function of the recorded seed (the portable PRNG of the test oracle `O`)."""
    xs = [O.portable_normal(seed, (B, D), stream=20 + m) for m in range(M)]
    Ws = [O.portable_normal(seed, (C, D), stream=30 + m, std=0.05) for m in range(M)]
    bs = [O.portable_normal(seed, (C,), stream=40 + m, std=0.1) for m in range(M)]
    return xs, Ws, bs


HEAD_CASES = [(2, 5, 512, 6, 11), (3, 4, 768, 4, 9), (2, 3, 768, 101, 7), (2, 1, 512, 6, 3), (2, 64, 512, 6, 70001)]
FORMS = {"av": (1.0, 0.1), "m3ae": (0.0, 1.0)}           # (w_cml, w_crl): main.py:265-268 | :203, 229


def case_tag(shape, form):
    return "head." + "_".join(str(v) for v in shape) + "." + form


def fixture_close(fx, key, got, rel, name=""):
    """|got - recorded| <= rel * max|recorded| for a fixture entry recorded whole, or as sampled positions per modality plus the
    sum of absolute values (make_golden_qmf.py: put).  Prints the figure before it asserts."""
    got = torch.as_tensor(got).detach().double().cpu().numpy()
    if key in fx:
        want = np.asarray(fx[key], dtype=np.float64)
        assert got.shape == want.shape, f"{name or key}: shape {got.shape} vs {want.shape}"
    else:
        pos, want = fx[key + ".pos"], np.asarray(fx[key + ".sub"], dtype=np.float64)
        total = float(fx[key + ".abssum"])
        got_sum = float(np.abs(got).sum())
        assert abs(got_sum - total) <= rel * total, f"{name or key}: abs-sum {got_sum} vs {total}"
        got = got.reshape(got.shape[0], -1)[:, pos]
    err = float(np.abs(got - want).max()) if want.size else 0.0
    bound = rel * float(np.abs(want).max()) if want.size else 0.0
    print(f"{name or key}: max|d| {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{name or key}: max|d|={err:.3e} > {bound:.3e}"
