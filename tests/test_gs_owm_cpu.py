"""CPU: the scalar-denominator head projector (gs_mode="owm").  The restatement of tests/owm_model.py has the properties the rule
is offered for, the two exact cases are exact (fp32 == fp64), the two ABI entries refuse bad arguments before anything is launched
(nothing is dereferenced), the workspace sizes match their formulas, GSPlugin takes the mode, and `make host-check` builds and runs
the host half's stand-alone sanitizer program."""
import ctypes
import os
import subprocess

import pytest
import torch

import owm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 65, 257])
def test_restatement_properties_over_free_running_calls(D):
    """40 calls from the identity on mixed-sign feature means, in fp64: Pl stays symmetric (bit for bit: the element update is
    symmetric in (i, j)), its eigenvalues stay in [0, 1] (a few ulp of slack for the eigensolver), Pl_new r = k alpha / s, s >= alpha."""
    for Pl, r, alpha, new, k, s in M.owm_run(D, 40):
        assert torch.equal(new, new.t())
        ev = torch.linalg.eigvalsh(new)
        assert ev.min().item() >= -1e-12 and ev.max().item() <= 1.0 + 1e-12, (ev.min().item(), ev.max().item())
        assert s.item() >= alpha * (1 - 1e-12)
        want = k * alpha / s
        assert (new @ r - want).abs().max().item() <= 1e-11 * max(k.abs().max().item(), 1e-300), D
    # a zero feature mean leaves Pl as it is: k = 0, s = alpha
    new, G, k, s = M.owm_ref(Pl, torch.zeros(D), torch.ones(3, D), 0.1)
    assert torch.equal(new, Pl) and s.item() == 0.1 and not k.any()
    assert torch.equal(G, torch.ones(3, D, dtype=torch.float64) @ Pl.t())


@pytest.mark.parametrize("zero_r", [False, True])
def test_exact_cases_are_exact(zero_r):
    """Both calls: s = 1, and Pl and G in fp32 equal Pl and G in fp64 bit for bit -- so the device must too."""
    c32, c64 = M.exact_case(torch.float32, zero_r), M.exact_case(torch.float64, zero_r)
    Pl0, G0, _rs = M.exact_inputs()
    for call, ((Pl32, G32, s32), (Pl64, G64, s64)) in enumerate(zip(c32, c64)):
        assert s64.item() == (M.EXACT_CALLS[call][1] if zero_r else 1.0) and s32.item() == s64.item()
        assert torch.equal(Pl32.double(), Pl64) and torch.equal(G32.double(), G64), call
        assert torch.equal(Pl64, Pl64.t())
        if zero_r:
            assert torch.equal(Pl64, Pl0.double()) and torch.equal(G64, G0.double())
        else:
            assert not torch.equal(G64, G0.double())
    if not zero_r:
        assert not torch.equal(c64[1][0], c64[0][0])          # the second call starts from, and moves, a non-identity Pl


def test_owm_phase_skips_the_first_call_and_counts_as_the_reference():
    import clip_model as R
    from oracle import mla_oracle as O
    B, D, C = 5, 70, 6
    st = R.ClipState({k: v.double() for k, v in O.make_head_params(D, C, 3).items()}, D)
    for ph in range(2):
        X = O.portable_normal(3 + ph, (B, D), stream=21, mean=0.3, std=0.7).double()
        out = M.owm_phase(st, X, O.portable_labels(3 + ph, B, C), ph, 5)
        assert st.exp_count == ph + 1
        assert torch.equal(out["grad"], out["grad_raw"]) == (ph == 0)
        assert torch.equal(st.Pl, torch.eye(D, dtype=torch.float64)) == (ph == 0)


# ---- the ABI without a GPU ------------------------------------------------------------------------------------------------------------
FAKE = [0x10000 * (i + 1) for i in range(9)]          # non-null, 16-byte aligned, far apart, never dereferenced


def _lib():
    from mla_hip import _lib
    return _lib.load()


def _refused(fn, text, *args):
    lib = _lib()
    assert getattr(lib, fn)(*args) == -1, f"{fn}{args} was not refused"
    msg = lib.mla_last_error().decode()
    assert fn + ":" in msg and text in msg, msg


def test_gs_project_owm_refuses_before_any_launch():
    Pl, r, G, ws = FAKE[:4]
    for z in range(4):
        a = [Pl, r, G, ws]
        a[z] = None
        _refused("mla_gs_project_owm", "null pointer", a[0], a[1], a[2], 64, 5, 0.1, a[3], None)
    _refused("mla_gs_project_owm", "need D, C > 0 (got 0, 5)", Pl, r, G, 0, 5, 0.1, ws, None)
    _refused("mla_gs_project_owm", "need D, C > 0 (got -3, 5)", Pl, r, G, -3, 5, 0.1, ws, None)
    _refused("mla_gs_project_owm", "need D, C > 0 (got 64, 0)", Pl, r, G, 64, 0, 0.1, ws, None)
    _refused("mla_gs_project_owm", "need D <= 8192 (got 8193)", Pl, r, G, 8193, 5, 0.1, ws, None)
    _refused("mla_gs_project_owm", "4-byte aligned", Pl + 2, r, G, 64, 5, 0.1, ws, None)
    _refused("mla_gs_project_owm", "overlaps", Pl, r, G, 64, 5, 0.1, G + 4 * 64, None)


def test_feature_phase_owm_refuses_before_any_launch():
    X, lab, W, b, buf, Pl, lg, loss, ws = FAKE
    tail = (1.0, 1, 0.1, 1e-3, 0.9, 1e-4, 1, None)
    for z in range(9):
        a = list(FAKE)
        a[z] = None
        _refused("mla_feature_phase_owm", "null pointer", *a, 2, 64, 5, *tail)
    assert _lib().mla_feature_phase_owm(X, lab, W, b, buf, None, lg, loss, None, 2, 64, 5, 1.0, 0, 0.1, 1e-3, 0.9, 1e-4, 1, None) == -1
    _refused("mla_feature_phase_owm", "need B, D, C > 0 (got 2, 0, 5)", *FAKE, 2, 0, 5, *tail)
    _refused("mla_feature_phase_owm", "need B, D, C > 0 (got 2, 64, -1)", *FAKE, 2, 64, -1, *tail)
    _refused("mla_feature_phase_owm", "need B, D, C > 0 (got 0, 64, 5)", *FAKE, 0, 64, 5, *tail)
    _refused("mla_feature_phase_owm", "need 0 < C <= 128 (got 129)", *FAKE, 2, 64, 129, *tail)
    _refused("mla_feature_phase_owm", "need D <= 4096 (got 4097)", *FAKE, 2, 4097, 5, *tail)
    _refused("mla_feature_phase_owm", "16-byte aligned", X, lab, W, b, buf, Pl + 4, lg, loss, ws, 2, 64, 5, *tail)
    # the literal phase still speaks under its own name
    _refused("mla_feature_phase", "need D <= 4096 (got 4097)", *FAKE, 2, 4097, 5, *tail)


def test_workspace_sizes_match_their_formulas():
    lib = _lib()
    from mla_hip import ops
    for D, C in ((1, 1), (64, 5), (70, 130), (257, 101), (768, 101), (8192, 128)):
        assert lib.mla_gs_owm_ws_elems(D, C) == D + C * D == ops.gs_owm_ws_elems(D, C)
    assert lib.mla_gs_owm_ws_elems(0, 5) == 0 and lib.mla_gs_owm_ws_elems(64, -1) == 0
    for B, D, C in ((1, 64, 1), (5, 70, 6), (64, 257, 101), (65, 64, 128)):          # the fused phase shares mla_feature_phase's workspace
        assert lib.mla_feature_ws_elems(B, D, C) == ((B * C + B + 3) & ~3) + 6 * D + C * D
    assert lib.mla_abi_version() == 3                                                 # the change is additive


# ---- Python -----------------------------------------------------------------------------------------------------------------------------
def test_gsplugin_takes_the_mode(monkeypatch):
    from mla_hip import GSPlugin
    g = GSPlugin(dim=8, device="cpu", mode="owm")
    assert g.mode == "owm" and g.exp_count == 0 and torch.equal(g.Pl, torch.eye(8))
    monkeypatch.setenv("MLA_GS_MODE", "owm")
    assert GSPlugin(dim=8, device="cpu").mode == "owm"
    assert GSPlugin(dim=8, device="cpu", mode="as_intended").mode == "as_intended"
    monkeypatch.delenv("MLA_GS_MODE")
    assert GSPlugin(dim=8, device="cpu").mode == "as_intended"                        # the default is untouched
    for bad in ("OWM", "scalar", "as-intended"):
        with pytest.raises(ValueError, match="mode must be"):
            GSPlugin(dim=8, device="cpu", mode=bad)
    g.before_update(None, None, 0, 10, 0)                                             # the first call is skipped: nothing is touched
    assert torch.equal(g.Pl, torch.eye(8))


def test_ops_and_torch_ops_are_there():
    import inspect
    from mla_hip import ops, torch_ops  # noqa: F401
    assert inspect.signature(ops.feature_phase).parameters["owm"].default is False
    assert callable(ops.gs_project_owm) and callable(ops.gs_owm_ws_elems)
    assert hasattr(torch.ops.mla_hip, "gs_project_owm") and hasattr(torch.ops.mla_hip, "gs_project")


def test_host_check_builds_and_runs_the_gs_program():
    csrc = os.path.join(ROOT, "multimodal-learning-with-alternating-unimodal-adaptation_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "host-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gs host check ok" in r.stdout and "gs_host_check.cpp" in r.stdout and "-fsanitize=address,undefined" in r.stdout
