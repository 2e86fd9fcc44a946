"""The scalar-denominator head projector (gs_mode="owm"; csrc/gs_owm.hip, mla_feature_phase_owm) restated on the CPU, for the tests.

  owm_ref      the rule on tensors of any dtype (fp64 by default): k = Pl r, s = alpha + r . k, Pl <- Pl - k k^T / s, G <- G Pl^T
  owm_run      free-running calls from the identity (the property tests)
  exact_case   the two calls on which fp32 and fp64 agree bit for bit (every value is a small multiple of a power of two, s = 1)
  dense_case   tests/tail_model.gs_case's inputs with this rule's fp64 references, two consecutive calls
  owm_phase    one whole head-only modality phase (main.py:432-442) with this rule: head, CE, dW / db, projection, SGD, in the dtype
               of the state it is handed (tests/clip_model.ClipState)

Only utils/utils.py:36-40 differ from the reference: the first call is skipped, alpha = 0.1 ** (batch_index / len_dataloader + 1),
r = mean(X, 0), the update comes before the projection, grad <- grad Pl^T, exp_count is counted as before."""
import functools
from types import SimpleNamespace

import torch

from oracle import mla_oracle as O
import tail_model as T

GS_RTOL = T.GS_RTOL                    # of max |want|: the project's GS tolerance


def owm_ref(Pl, r, G, alpha, dtype=torch.float64):
    """(Pl_new, G_new, k, s) in `dtype`.  The element update is Pl[i][j] - (k_i * k_j) / s, as the kernels form it."""
    Pl, r, G = Pl.to(dtype), r.to(dtype).reshape(-1), G.to(dtype)
    k = Pl @ r
    s = torch.as_tensor(alpha, dtype=dtype) + r @ k
    Pl = Pl - torch.outer(k, k) / s
    return Pl, G @ Pl.t(), k, s


def feature_means(D, calls, seed, scale=1.0):
    """Mixed-sign feature means, one per call: unit normals times `scale`."""
    return [O.portable_normal(seed + D, (D,), stream=30 + c) * scale for c in range(calls)]


def owm_run(D, calls, seed=900, dtype=torch.float64):
    """Free-running calls from the identity with alpha as a 10-batch epoch gives it: [(Pl_before, r, alpha, Pl_after, k, s)]."""
    Pl, out = torch.eye(D, dtype=dtype), []
    G = torch.zeros((1, D), dtype=dtype)
    for c, r in enumerate(feature_means(D, calls, seed)):
        alpha = O.gs_alpha(c % 10, 10)
        new, _G, k, s = owm_ref(Pl, r, G, alpha, dtype)
        out.append((Pl, r.to(dtype), alpha, new, k, s))
        Pl = new
    return out


# ---- the exact case ------------------------------------------------------------------------------------------------------------------
EXACT_D, EXACT_C = 64, 5
EXACT_CALLS = (((1, 17, 63), 0.25), ((1, 2, 5), 0.3125))          # (where r = 0.5, alpha): s = 1 in both calls


def exact_inputs():
    """Pl = I, G integers in [-8, 8], and the two feature means."""
    G = torch.from_numpy(T._ints(77, EXACT_C * EXACT_D, -8, 8).astype("float32")).view(EXACT_C, EXACT_D)
    rs = []
    for where, _alpha in EXACT_CALLS:
        r = torch.zeros(EXACT_D)
        r[list(where)] = 0.5
        rs.append(r)
    return torch.eye(EXACT_D), G, rs


def exact_case(dtype=torch.float64, zero_r=False):
    """[(Pl, G, s) after each of the two calls] in `dtype`; zero_r: r = 0 instead (k = 0: Pl and G must not move)."""
    Pl, G, rs = exact_inputs()
    out = []
    for r, (_where, alpha) in zip(rs, EXACT_CALLS):
        Pl, G, _k, s = owm_ref(Pl, torch.zeros_like(r) if zero_r else r, G, alpha, dtype)
        out.append((Pl, G, s))
    return out


# ---- dense against fp64 ---------------------------------------------------------------------------------------------------------------
DENSE_ALPHAS = (1.0, 0.01)


@functools.lru_cache(maxsize=None)
def dense_case(D, C, alpha):
    """tail_model.gs_case's Pl = I, feature means and G; the fp64 references of two consecutive calls of this rule (the second starts
    from the fp32 rounding of the first, as the device does)."""
    c = T.gs_case(D, C)
    Pl1, G1, _k, _s = owm_ref(torch.eye(D), c.rs[0], c.G, alpha)
    Pl2, G2, _k, _s = owm_ref(Pl1.float(), c.rs[1], G1.float(), alpha)
    return SimpleNamespace(D=D, C=C, rs=c.rs, G=c.G, want=[(Pl1, G1), (Pl2, G2)])


# ---- one whole feature phase ----------------------------------------------------------------------------------------------------------
def owm_phase(st, X, label, batch_index, len_dataloader, lr=1e-3, momentum=0.9, wd=1e-4):
    """main.py:432-442 on the state, in place, with the scalar-denominator rule in GSPlugin.before_update's place.  Returns logits, loss,
    the raw and the projected weight gradient and the bias gradient."""
    W, b = st.head["weight"], st.head["bias"]
    logits, loss, dW, db, _dX = O.head_ce_fwd_bwd(X, W, b, label)                # :432-435
    raw = dW.clone()
    if st.exp_count != 0:                                                        # utils/utils.py:29 (the first call is skipped)
        st.Pl, dW, _k, _s = owm_ref(st.Pl, X.mean(dim=0), dW, O.gs_alpha(batch_index, len_dataloader), X.dtype)
    st.head["weight"], st.mom["weight"] = O.sgd_step(W, dW, st.mom["weight"], lr, momentum, wd)           # :439
    st.head["bias"], st.mom["bias"] = O.sgd_step(b, db, st.mom["bias"], lr, momentum, wd)
    st.exp_count += 1                                                            # :442
    return {"out": logits, "loss": loss, "grad_raw": raw, "grad": dW, "bias_grad": db}
