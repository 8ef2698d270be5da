"""CPU self-test of tests/ipa_ref.py and of the case table of tests/test_ipa_attention_gpu.py.

(a) `core` is the oracle's IPA between the input projections and linear_out (fp64, 1e-12); the oracle is pinned to the reference
by the goldens.  (b) Through `mdgen_debug_ipa_slices` (host only), every case of the GPU test gets the forward kernel and the
slice counts its comment claims, and the table holds what it aims at.  (c) The floor-relative gate on a stand-in device -- `core`
in torch fp32: clean, it passes every gate of every case; with one key dropped, one padded key attended, one 32-key slice left
out of the merge, the softplus threshold branch wrong or the frames of a group taken from the wrong sample, it exceeds the gate
of every affected quantity at least ten times.
"""
import ctypes as C

import pytest
import torch

import ipa_ref as IR
from oracle import mdgen_oracle as O

IDS = [c.id for c in IR.CASES]


def test_core_is_the_oracles_ipa():
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_state_dict
    B, L = 3, 37
    cfg = ModelConfig.forward_sim(num_frames=2, crop=L)
    pre = "ipa_layers.0.ipa."
    P = {k: v.double() for k, v in synth_state_dict(cfg, 5).items() if k.startswith(pre)}
    P[pre + "head_weights"] = torch.tensor(IR.HEAD_W).double()
    inp = IR.inputs(B, B, L, "chain", 11)
    gen = torch.Generator().manual_seed(3)
    s = torch.randn(B, L, 384, generator=gen).double()
    R, t, mask = inp["rot"].double(), inp["trans"].double(), inp["mask"].double()
    want = O.ipa(P, pre, s, R, t, mask)
    proj = torch.cat([O.linear(P, pre + n, s) for n in ("linear_q", "linear_kv", "linear_q_points", "linear_kv_points")], -1)
    feat, lse = IR.core(proj.reshape(B * L, 672), R, t, mask, P[pre + "head_weights"])
    got = O.linear(P, pre + "linear_out", feat.view(B, L, 256))
    assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    assert torch.isfinite(lse).all()


def _slices(c):
    import mdgen_amd._lib as L
    f, b, t = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib.mdgen_debug_ipa_slices(c.ngroups, c.L, int(c.scratch is not None), c.part_floats, C.byref(f), C.byref(b), C.byref(t)))
    return f.value, b.value, bool(t.value)


@pytest.mark.parametrize("case", IR.CASES, ids=IDS)
def test_case_gets_the_kernel_and_the_slices_its_comment_claims(case):
    f, b, tiled = _slices(case)
    assert tiled == case.tiled == (case.L >= 24)
    assert (f, IR.slices_used(case.L, f)[1]) == case.fwd
    if case.bwd is not None:
        assert (b, IR.slices_used(case.L, b)[1]) == case.bwd
        assert case.ngroups == case.B                     # the hook refuses a backward otherwise: not a product call
    # what the scratch must hold for these counts fits it (the device writes exactly this much)
    M = case.ngroups * case.L
    if f > 1:
        assert f * M * IR.FWD_REC <= case.part_floats
    if b > 1:
        assert b * M * IR.BWD_ROW <= case.part_floats


def test_case_table_holds_what_it_aims_at():
    import mdgen_amd._lib as L
    cs = IR.CASES
    assert len(set(IDS)) == len(IDS)
    assert {c.tiled for c in cs} == {False, True}
    for d in ("fwd", "bwd"):
        got = [getattr(c, d) for c in cs if getattr(c, d) is not None]
        assert any(n == 1 for n, _ in got) and any(n > 1 for n, _ in got), d
        assert sum(1 for _, e in got if e > 0) >= 2, d
    for kind in ("compact", "chain"):
        assert {(c.B, c.L) for c in cs if c.kind == kind} >= {(4, 130), (3, 200), (6, 100)}
    assert {c.L for c in cs if c.ngroups == c.B and c.scratch == "full" and c.B <= 2} >= {1, 5, 23, 24, 31, 32, 33, 64, 65, 255, 256, 257, 300}
    assert {(c.ngroups, c.B, c.L) for c in cs if c.bwd is None} == {(6, 2, 33), (4, 1, 257)}
    # the scratch limits at B 1, L 257: one that cuts a slice count, one that cuts it to 1, and NULL
    full = _slices(IR.Case(1, 1, 257, "compact", "full", True, None, None))[:2]
    lim = [(c, _slices(c)[:2]) for c in cs if (c.ngroups, c.B, c.L) == (1, 1, 257) and c.scratch != "full"]
    assert any(c.scratch is None for c, _ in lim)
    for d in (0, 1):
        assert any(c.scratch and 1 < s[d] < full[d] for c, s in lim), d
        assert any(c.scratch and s[d] == 1 < full[d] for c, s in lim), d
    # the hook's argument checks need no device: a backward with ngroups != B, and null pointers
    one = C.c_int32()
    p = C.c_void_p(256)   # (never dereferenced: refused before any launch)
    assert L.lib.mdgen_debug_ipa_attention(p, p, p, p, p, 4, 2, 8, None, 0, p, p, None, p, p, p, p, C.byref(one), C.byref(one), None) == -2
    assert L.lib.mdgen_debug_ipa_attention(None, p, p, p, p, 2, 2, 8, None, 0, None, p, None, p, None, None, None, C.byref(one), C.byref(one), None) == -1
    assert L.lib.mdgen_debug_ipa_attention(p, p, p, p, p, 2, 2, 8, None, 0, p, p, None, p, None, p, p, C.byref(one), C.byref(one), None) == -1
    assert L.lib.mdgen_debug_ipa_slices(0, 8, 1, 0, C.byref(one), C.byref(one), C.byref(one)) == -2


# ---- faults on the stand-in ---------------------------------------------------------------------------------------------------
def _first(cond):
    return int(torch.nonzero(cond)[0])


def _faults(case, inp):
    """{name: (hooks, affected quantities)} of the faults that exist in this case."""
    B, L, G = case.B, case.L, case.ngroups
    mask = inp["mask"]
    out = {}
    bq = ("feat", "lse", "dproj") if case.bwd is not None else ("feat", "lse")
    g = G - 1                       # the last group: the last sample, whose tail is padded
    b = g % B
    if mask[b].sum() >= 2:
        j = _first(mask[b] > 0)

        def dropped(raw, mterm, h, j=j):
            lg = raw + mterm
            if h == 0:
                lg = lg.clone()
                lg[g, :, j] = float("-inf")
            return lg
        out["one real key dropped"] = ({"logits": dropped}, bq)
    if mask[b].sum() >= 2 and (mask[b] == 0).any():
        j = _first(mask[b] == 0)

        def attended(raw, mterm, h, j=j):
            if h == 0:
                mterm = mterm.clone()
                mterm[g, mask[b] > 0, j] = 0.0
            return raw + mterm
        out["one padded key attended"] = ({"logits": attended}, bq)
    if case.fwd[0] > 1:
        def unmerged(raw, mterm, h):
            lg = (raw + mterm).clone()
            lg[:, :, 0:32] = float("-inf")
            return lg
        out["a 32-key slice left out of the merge"] = ({"logits": unmerged}, bq)
    # softplus(25) without the threshold, log1p(exp(25)), IS 25 in fp32: leaving the branch out is no fault that any test
    # could see (asserted below).  What can go wrong is the branch itself: here it returns the threshold instead of w.
    out["softplus: the threshold returned above it"] = (
        {"softplus": lambda w: torch.where(w > 20, torch.full_like(w, 20.0), torch.log1p(torch.exp(w)))},
        ("feat", "lse", "dhead_w") if case.bwd is not None else ("feat", "lse"))
    if G > B > 1:
        out["frames of group g from sample g // (ngroups / B)"] = ({"frames": lambda G_, B_: torch.arange(G_) // (G_ // B_)}, ("feat", "lse"))
    return out


def test_softplus_without_its_threshold_is_the_same_number_in_fp32():
    with torch.enable_grad():
        w = torch.tensor(IR.HEAD_W, requires_grad=True)
        a = torch.nn.functional.softplus(w)
        b = torch.log1p(torch.exp(w))
        ga, = torch.autograd.grad(a.sum(), w)
        gb, = torch.autograd.grad(b.sum(), w)
    assert a[3] == b[3] == 25.0
    assert ga[3] == gb[3] == 1.0


@pytest.mark.parametrize("case", IR.CASES, ids=IDS)
def test_gate_passes_the_clean_standin_and_catches_faults(case):
    inp, ref, gate, floor = IR.reference(case)
    bwd = case.bwd is not None
    print(IR.report_line(case.id, floor, floor))
    IR.check(case.id, floor, gate)      # the clean stand-in's metric IS the floor: under 32 x itself by construction
    if case.kind != "compact" or case.L < 5:
        return
    for name, (hooks, affected) in _faults(case, inp).items():
        got = IR.metrics(IR.run_core(inp, torch.float32, bwd, hooks), ref, inp)
        print(f"  {name}: " + ", ".join(f"{k} {got[k][0]:.2e} (gate {gate[k][0]:.2e})" for k in affected))
        for k in affected:
            assert got[k][0] > 10 * gate[k][0], (case.id, name, k, got[k], gate[k])


def test_every_fault_is_applied_somewhere():
    names = set()
    for c in IR.CASES:
        if c.kind == "compact" and c.L >= 5:
            names |= set(_faults(c, IR.inputs(c.B, c.ngroups, c.L, c.kind, c.seed)))
    assert len(names) == 5, names
