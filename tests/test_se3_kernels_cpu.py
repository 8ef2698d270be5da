"""CPU self-test of tests/se3_ref.py and of the case table of tests/test_se3_kernels_gpu.py.

(a) The reference functions of se3_ref, in the form the GPU test calls them, reproduce the reference's own goldens (rigid_ops,
geometry, prep_sim, prep_tps, prep_sim_interval).  (b) The case table holds what it aims at, and `reference` finds its conditions
met in every case: no quaternion takes the sign-free path outside the pi families, every torsion kind is compared on at least four
residues and 60 % of all torsion entries are.  (c) The floor-relative gates and the exact assertions on a stand-in device -- the
oracle in torch fp32: clean, it passes every case; with each of the faults of FAULTS it misses a gate or an exact assertion in every
case the fault exists in.
"""
from unittest import mock

import pytest
import torch

import se3_ref as SR
from conftest import load_golden
from oracle import mdgen_oracle as O

torch.set_grad_enabled(False)
IDS = [c.id for c in SR.CASES]
F64 = torch.float64


# ---- (a) the references against the goldens ------------------------------------------------------------------------------------
def _close(a, b, atol):
    return float((a.double() - b.double()).abs().max()) <= atol


def test_algebra_reference_reproduces_the_rigid_ops_golden():
    g = load_golden("rigid_ops")
    inp = dict(R1=g["R1"], R2=g["R2"], t1=g["t1"], t2=g["t2"], p=g["p"], q=g["q7"][:, :4].contiguous(), p3a=g["p3a"], p3b=g["p3b"], p3c=g["p3c"])
    out = SR.oracle(SR.Case("algebra", n=64), inp, F64)
    for k, gk, atol in (("comp_R", "comp_R", 1e-6), ("comp_t", "comp_t", 1e-5), ("inv_R", "inv_R", 0.0), ("inv_t", "inv_t", 1e-5),
                        ("apply", "apply", 1e-5), ("inv_apply", "invert_apply", 1e-5), ("q2r_norm", "from7_R", 1e-6), ("f3_R", "f3_R", 1e-6),
                        ("f3_t", "f3_t", 0.0)):
        assert _close(out[k], g[gk], atol), k
    (e, _), _ = SR._quat(out["quat"], g["tensor7"][:, :4], None)       # the golden's sign is eigh's: arbitrary
    assert e < 1e-5
    assert float(out["ident_t"].abs().max()) < 1e-6 * float(g["t1"].abs().max())     # (R1 is orthogonal to fp32 rounding only)
    ap = SR.oracle(SR.Case("apply", n=64, ppf=1), dict(R=g["R1"], t=g["t1"], p=g["p"][:, None]), F64)
    assert _close(ap["apply"][:, 0], g["apply"], 1e-5) and _close(ap["inv_apply"][:, 0], g["invert_apply"], 1e-5)
    r2q = SR.oracle(SR.Case("r2q", family="random"), dict(R=g["R1"]), F64)
    assert torch.equal(r2q["quat"], out["quat"])


def test_cond_and_post_references_reproduce_the_geometry_golden():
    g = load_golden("geometry")
    B, T, L = g["atom14"].shape[:3]
    sq = g["seqres"][:, None].expand(B, T, L).reshape(B * T, L)
    c = SR.Case("cond", B=B * T, L=L, centre=0)
    tm = g["torsion_mask"].reshape(B * T, L, 7)
    # (the golden's torsions are the reference's fp32: R^T p - R^T t, which cancels at the size of the coordinates; the fp64 run
    # is 1e-5 .. 1e-4 away from them, the fp32 run of the same function as close as test_oracle_cpu.py asks)
    for dt, atol in ((torch.float32, 1e-5), (F64, 1e-4)):
        out = SR.oracle(c, dict(atom14=g["atom14"].reshape(B * T, L, 14, 3), seqres=sq), dt)
        assert _close(out["rots"], g["frames_R"].reshape(B * T, L, 3, 3), 1e-5) and _close(out["trans"], g["frames_t"].reshape(B * T, L, 3), 0.0)
        assert torch.equal(out["torsion_mask"].float(), tm)
        assert _close(out["torsions"] * tm[..., None], g["torsions"].reshape(B * T, L, 7, 2) * tm[..., None], atol), dt
    # frames + torsions -> atom14 through the post-processing with identity offsets, one frame per "sample"
    s = torch.zeros(B * T, 1, L, 21)
    s[..., 0] = 1.0
    s[..., 7:] = g["torsions"].reshape(B * T, 1, L, 14)
    p = SR.Case("post", B=B * T, T=1, L=L, tps=0)
    back = SR.oracle(p, dict(samples=s, rot0=g["frames_R"].reshape(B * T, L, 3, 3), trans0=g["frames_t"].reshape(B * T, L, 3), seqres=sq), F64)
    assert _close(back["atom14"][:, 0], g["atom14_back"].reshape(B * T, L, 14, 3), 1e-4)


@pytest.mark.parametrize("name", ["prep_sim", "prep_tps", "prep_sim_interval"])
def test_prep_reference_reproduces_the_prep_goldens(name):
    g = load_golden(name)
    B, T, L = g["in_trans"].shape[:3]
    c = SR.Case("prep", B=B, T=T, L=L, tps=int(g["cfg"]["tps_condition"]), ci=int(g["cond_interval"]))
    inp = dict(rots=g["in_rots"], trans=g["in_trans"], torsions=g["in_torsions"], seqres=g["in_seqres"])
    for dt, atol in ((F64, 2e-5), (torch.float32, 2e-5)):
        out = SR.oracle(c, inp, dt)
        assert _close(out["latents"], g["latents"], atol) and _close(out["x_cond"], g["x_cond"], atol)
        assert torch.equal(out["x_cond_mask"], g["x_cond_mask"])


# ---- (b) the case table --------------------------------------------------------------------------------------------------------
def test_case_table_holds_what_it_aims_at():
    cs = SR.CASES
    assert len(set(IDS)) == len(IDS)
    by = lambda grp: [c for c in cs if c.group == grp]
    assert [c.n for c in by("algebra")] == [1, 255, 256, 257, 513]
    assert {(c.n, c.ppf) for c in by("apply")} == {(257, 1), (19, 14), (7, 37)}
    assert all(c.n * c.ppf > 256 and (c.ppf == 1 or 256 % c.ppf) for c in by("apply"))      # a block boundary inside a frame
    assert {c.family for c in by("r2q")} == {"random", "pi", "pi-1e-07", "pi-0.0001", "pi-0.01", "small", "dom_w", "dom_x", "dom_y", "dom_z",
                                             "relative"}
    for c in by("r2q"):
        assert SR.reference(c)[0]["R"].shape == (257, 3, 3)
    for B, T, L in ((2, 5, 3), (1, 1, 4), (3, 7, 37)):
        for tps in (0, 1):
            assert {c.ci for c in by("prep") if (c.B, c.T, c.L, c.tps) == (B, T, L, tps)} == {0, 1, 3, T, T + 5}
    assert {(c.B, c.T, c.L, c.tps) for c in by("post")} == {(B, T, L, tps) for B, T, L in ((2, 3, 23), (1, 13, 20)) for tps in (0, 1)}
    assert {(c.B, c.L, c.centre) for c in by("cond")} == {(B, L, x) for B, L in ((3, 23), (1, 300)) for x in (0, 100)}
    assert {(c.gvp, c.per) for c in by("plan")} == {(g, p) for g in (0, 1) for p in (1, 255, 257, 630)}
    assert SR.PLAN_T[0] == 0.0 and SR.PLAN_T[-1] == 1.0
    assert [c.per for c in by("mse")] == [1, 255, 256, 257, 1792, 1793, 2047, 2048, 2049, 4113, 27720]


def test_inputs_are_what_the_case_table_says():
    by = lambda grp: [c for c in SR.CASES if c.group == grp]
    for c in by("algebra"):
        inp = SR.reference(c)[0]
        assert 50 < float(inp["t1"].abs().max()) or c.n == 1
        nq = inp["q"].double().norm(dim=-1)
        assert c.n < 255 or (float(nq.min()) < 1e-2 and float(nq.max()) > 1e2)
        assert torch.equal(inp["p3a"][-1], inp["p3b"][-1]) and torch.equal(inp["p3c"][-1], inp["p3b"][-1])
    for c in by("r2q"):
        inp, ref, gate, _ = SR.reference(c)
        w = ref["quat"][:, 0].abs()
        if c.family in ("pi", "pi-1e-07"):
            assert float(w.max()) <= gate["quat"][0]                   # every frame on the sign-free path
            q = ref["quat"][:6, 1:].abs()
            assert bool(((q - torch.eye(3).repeat(2, 1).double()).abs() < 1e-6).all())
        elif c.family in SR.PI_FAMILIES:
            assert float(w.min()) > gate["quat"][0] and float(w.max()) < 1e-2
        elif c.family == "small":
            assert float(w.min()) > 1 - 1e-8 and torch.equal(inp["R"][0], torch.eye(3))
        elif c.family.startswith("dom_"):
            assert bool((ref["quat"].abs().argmax(-1) == "wxyz".index(c.family[-1])).all())
        elif c.family == "relative":
            RtR = torch.einsum("nji,njk->nik", inp["R"].double(), inp["R"].double())
            assert 1e-8 < float((RtR - torch.eye(3).double()).abs().max()) < 1e-5
    for c in by("prep"):
        inp, ref, gate, _ = SR.reference(c)
        if c.T > 1:
            assert float(ref["latents"][:, 1, :, 0].abs().max()) <= gate["quat0"][0]     # the frame turned by pi: w ~ 0
    for c in by("post"):
        inp = SR.reference(c)[0]
        sq = inp["seqres"]
        assert set(sq.flatten().tolist()) >= set(range(1, 21)) and 20 in sq and (c.L < 21 or 0 in sq)
        assert c.B == 1 or not bool((sq[0] == sq[1]).any())
        assert c.B == 1 or float((inp["rot0"][0] - inp["rot0"][1]).abs().max()) > 0.1
        assert float(inp["trans0"].abs().mean()) > 80
        D = inp["samples"].shape[-1]
        assert D == (28 if c.tps else 21)
        for n in (inp["samples"][..., :4].double().norm(dim=-1), inp["samples"][..., D - 14:].double().reshape(-1, 2).norm(dim=-1)):
            assert float(n.min()) < 0.03 and float(n.max()) > 30
    for c in by("cond"):
        inp = SR.reference(c)[0]
        assert set(inp["seqres"].flatten().tolist()) == set(range(21))
        assert abs(float(inp["atom14"][..., 1, :][inp["seqres"] != 20].mean()) - c.centre) < 3      # (type 20 has no atoms: zeros)
    for c in by("mse"):
        inp = SR.reference(c)[0]
        assert float(inp["mask_last"].sum()) == SR.MSE_B and bool((inp["mask_last"][:, -1] == 1).all())
        assert c.per < 255 or 0.6 < float(inp["mask_random"].mean()) < 0.8


# ---- (c) the stand-in: clean, and with faults ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SR.CASES, ids=IDS)
def test_fp32_oracle_passes_every_gate_and_exact_assertion(case):
    inp, ref, gate, floor = SR.reference(case)
    got, _ = SR.verify(case, SR.standin(case, inp))
    print(SR.report_line(case.id, got, floor))


def _negate_one_quat(key):
    def f(c, inp, out):
        ref = SR.reference(c)[1]
        q = out[key] if key == "quat" else out["latents"][..., :4]
        r = (ref[key] if key == "quat" else ref["latents"][..., :4]).reshape(-1, 4)
        q.view(-1, 4)[int(r[:, 0].abs().argmax())] *= -1            # |w_ref| there is far above the gate
        if "x_cond" in out:
            out["x_cond"] = torch.where(out["x_cond_mask"][..., None] == 1, out["latents"], torch.zeros(()))
        return out
    return f


def _compose_order(c, inp, out):
    out["comp_R"] = O.rot_matmul(inp["R2"], inp["R1"])
    return out


def _inv_t_sign(c, inp, out):
    out["inv_t"] = -out["inv_t"]
    return out


def _apply_mod_n(c, inp, out):
    return SR.standin(c, inp, frame_of=lambda n, ppf: torch.arange(n * ppf) % n)


def _nan_row_256(c, inp, out):
    """Row 256 (the first of the second block) of one output left as the fill: every output in turn."""
    muts = []
    for k in out:
        m = {kk: v.clone(memory_format=torch.contiguous_format) for kk, v in out.items()}
        rows = m[k].reshape(-1, m[k].shape[-1]) if c.group != "algebra" else m[k].reshape(c.n, -1)
        if rows.shape[0] > 256 and k != "ident_t":      # (ident_t is made from comp_t's kernel: covered there)
            rows[256] = float("nan")
            muts.append(m)
    return muts


def _recond(out):
    out["x_cond"] = torch.where(out["x_cond_mask"][..., None] == 1, out["latents"], torch.zeros(()))
    return out


def _tps_second_ref_frame0(c, inp, out):
    out["latents"][..., 7:14] = out["latents"][..., 0:7]
    return _recond(out)


def _flag_missing_last(c, inp, out):
    out["x_cond_mask"][:, -1] = 0
    return _recond(out)


def _ci_shifted(c, inp, out):
    t = torch.arange(c.T)
    out["x_cond_mask"][:] = ((t == 0) | (c.tps == 1) & (t == c.T - 1) | (t % c.ci == 1)).long()[None, :, None]
    return _recond(out)


def _x_cond_not_zeroed(c, inp, out):
    out["x_cond"] = out["latents"].clone()
    return out


def _torsions_not_normalised(c, inp, out):
    real = torch.linalg.norm
    with mock.patch.object(torch.linalg, "norm", lambda x, *a, **k: torch.ones_like(x[..., :1]) if x.shape[-1] == 2 else real(x, *a, **k)):
        return SR.standin(c, inp)


def _chi2_not_chained(c, inp, out):
    """O.rigid_compose is called six times by the post-processing: R0 o offset, default o torsion rotation, chi2 / chi3 / chi4 onto
    their predecessor, backbone o group.  The third call returns its second operand: chi2 stands on the backbone."""
    real, n = O.rigid_compose, [0]

    def patched(R1, t1, R2, t2):
        n[0] += 1
        return (R2, t2) if n[0] == 3 else real(R1, t1, R2, t2)
    with mock.patch.object(O, "rigid_compose", patched):
        res = SR.standin(c, inp)
    assert n[0] == 6
    return res


def _rot0_of_sample0(c, inp, out):
    return SR.standin(c, inp, rot0=lambda r: r[:1].expand_as(r))


def _tps_torsions_col7(c, inp, out):
    return SR.standin(c, inp, tps=0)


def _cross_sample_read(c, inp, out):
    return SR.standin(c, inp, view=(1, c.B * c.L))


def _psi_flip_missing(c, inp, out):
    out["torsions"][..., 2, :] *= -1
    return out


def _column_flip_missing(c, inp, out):
    out["rots"] = out["rots"] * torch.tensor([-1.0, 1.0, -1.0])
    return out


def _plan_t0(c, inp, out):
    return SR.standin(c, inp, t_of=lambda t: t[:1].expand_as(t).contiguous())


def _mse_drop_last(c, inp, out):
    return SR.standin(c, inp, loss_of=lambda x, m: O.mean_flat(x[:, :-1], m[:, :-1]))


def _mse_count_all(c, inp, out):
    return SR.standin(c, inp, loss_of=lambda x, m: (x * m).sum(1) / x.shape[1])


_prep_uncond = lambda c: c.T > 1 and c.ci != 1                       # some frame is no conditioning frame
# name: (mutation, the cases in which the fault exists)
FAULTS = {
    "one quaternion negated where |w| is above the gate": (_negate_one_quat("quat"), lambda c: c.group == "algebra" or (c.group == "r2q" and c.family not in ("pi", "pi-1e-07"))),
    "one offset quaternion of prep_latents negated": (_negate_one_quat("latents"), lambda c: c.group == "prep"),
    "R2 R1 instead of R1 R2": (_compose_order, lambda c: c.group == "algebra"),
    "the inverted translation with the wrong sign": (_inv_t_sign, lambda c: c.group == "algebra"),
    "rigid_apply frame index i % n": (_apply_mod_n, lambda c: c.group == "apply" and c.ppf > 1),
    "row 256 left as the NaN fill": (_nan_row_256, lambda c: (c.group == "algebra" and c.n > 256) or c.group in ("r2q", "apply")),
    "the second TPS reference taken as frame 0": (_tps_second_ref_frame0, lambda c: c.group == "prep" and c.tps and c.T > 1),
    "the conditioning flag missing at T - 1": (_flag_missing_last, lambda c: c.group == "prep" and c.tps and c.T > 1),
    "a cond_interval frame shifted by one": (_ci_shifted, lambda c: c.group == "prep" and 1 < c.ci < c.T),
    "x_cond not zeroed off-condition": (_x_cond_not_zeroed, lambda c: c.group == "prep" and _prep_uncond(c)),
    "torsion pairs not normalised": (_torsions_not_normalised, lambda c: c.group == "post"),
    "chi2 not chained onto chi1": (_chi2_not_chained, lambda c: c.group == "post"),
    "sample 0's rot0 used for every sample": (_rot0_of_sample0, lambda c: c.group == "post" and c.B > 1),
    "TPS torsions read at column 7": (_tps_torsions_col7, lambda c: c.group == "post" and c.tps),
    "residue 0 of sample 1 reading sample 0's last residue": (_cross_sample_read, lambda c: c.group == "cond" and c.B > 1),
    "the psi sign flip missing": (_psi_flip_missing, lambda c: c.group == "cond"),
    "the diag(-1, 1, -1) column flip missing": (_column_flip_missing, lambda c: c.group == "cond"),
    "sample 0's t used for all samples in path_plan": (_plan_t0, lambda c: c.group == "plan"),
    "masked_mse dropping its last element": (_mse_drop_last, lambda c: c.group == "mse"),
    "masked_mse counting every element in the denominator": (_mse_count_all, lambda c: c.group == "mse" and c.per > 1),
}


def _miss(case, out):
    try:
        SR.verify(case, out)
    except AssertionError as e:
        return str(e)[:160]
    return None


@pytest.mark.parametrize("name", list(FAULTS))
def test_fault_misses_a_gate_or_an_exact_assertion(name):
    mutate, exists = FAULTS[name]
    cases = [c for c in SR.CASES if exists(c)]
    assert cases, name
    for c in cases:
        inp = SR.reference(c)[0]
        outs = mutate(c, inp, {k: v.clone() for k, v in SR.standin(c, inp).items()})
        outs = outs if isinstance(outs, list) else [outs]
        assert outs, (name, c.id)
        for out in outs:
            why = _miss(c, out)
            assert why is not None, (name, c.id, "the fault passed")
        print(f"{name} | {c.id}: {why}")


def test_the_cross_sample_read_is_caught_by_the_mask_of_residue_0():
    """The assertion on the pre-omega / phi masks of residue 0 alone catches the read across the sample boundary."""
    for c in (c for c in SR.CASES if c.group == "cond" and c.B > 1):
        inp = SR.reference(c)[0]
        tm = SR.standin(c, inp, view=(1, c.B * c.L))["torsion_mask"]
        assert bool((tm[0, 0, :2] == 0).all()) and bool((tm[1:, 0, :2] == 1).all())
