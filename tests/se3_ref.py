"""The SE(3), pre/post-processing and loss kernels of csrc/k_se3.hip and csrc/k_small.hip (k_rigid_compose, k_rigid_invert,
k_rigid_apply, k_quat_to_rot, k_rot_to_quat, k_from_3_points, k_prep_latents, k_samples_to_atom14, k_atom14_to_cond, k_path_plan,
k_masked_mse; k_rel7's arithmetic through prep_latents(tps = 1) and rot_to_quat): the case table, the inputs, the fp64 references,
the metrics, the floor-relative gate and the exact assertions of tests/test_se3_kernels_{cpu,gpu}.py.

A test helper, not a test module.  The references are the oracle's own functions (oracle/mdgen_oracle.py, pinned to the reference's
goldens by test_oracle_cpu.py and again, in the form used here, by test_se3_kernels_cpu.py) run in fp64 on the device's own fp32
inputs.

The gate is not a fixed number.  For every case and quantity, `floor` is the metric of the same oracle function in torch fp32 on the
CPU against its fp64 result, and gate = max(32 * floor, 32 * 2^-24), both relative to the quantity's scale as ipa_ref._rows defines
it (rms over the rows of the fp64 result's row norm): 32 x for what a kernel legitimately does differently from torch's fp32 (another
summation order, another sqrt / division, a power iteration instead of eigh), 32 fp32 ulps of the scale for floors that happen to be
tiny or zero.

Quaternions (`_quat`): the reference is the fp64 eigenvector flipped to w >= 0.  Where |w_ref| is above the case's quaternion gate
the sign must match; at or below it both signs are as good as each other and the smaller of |q - q_ref| and |q + q_ref| counts.  The
floor itself is measured sign-free (eigh's sign is arbitrary).  Outside the pi families no frame may take the sign-free path:
`reference` asserts it.

Torsions of atom14_to_cond are compared where the fp64 torsion_mask is 1; masked slots are ill-conditioned (fp32 and fp64 differ by
O(1) there) and only have to be finite and of norm <= 1 + gate.  `reference` asserts that each of the 7 torsion kinds is compared on
at least 4 residues of a case and that at least 60 % of all torsion entries are.

Worst measured device / floor ratio per quantity and case family (row max | rel-L2), MI355X, against the factor 32:
  frame algebra, n 1 .. 513 (compose, invert, apply both ways, quat_to_rot raw / normalised, from_3_points, A o A^-1): 0.9 .. 1.1 | 1.0
      -- the kernels round like torch's fp32; the rotation of rigid_invert bit-exact, from_3_points' translation exact
  rigid_apply at (257, 1), (19, 14), (7, 37): 1.0 | 1.0
  rot_to_quat: 0.3 .. 0.4 | 0.4 .. 0.7 in every family (1.2e-7 .. 1.6e-7 of the fp64 eigenvector where torch's fp32 eigh has
      3.2e-7 .. 4.9e-7), at pi, near pi, with every component dominant and on R1^T R2 alike; angle <= 1e-4: 1.0 | 1.0 (1.2e-9)
  prep_latents: quaternions 0.2 .. 0.6 | 0.3 .. 0.5, translations 1.0 | 1.0; T = 1: both exactly the fp64 values
  samples_to_atom14: 1.0 | 1.0 (1.1e-7 .. 1.5e-7 of the 100 A scale)
  atom14_to_cond: rotations 1.2 | 1.1, translations exact; valid torsions, centre 0: 0.5 | 0.8 (B 3, L 23), 2.2 | 3.3 (B 1, L 300);
      centre 100 A: 8.8 | 20.0 (B 3, L 23), 18.1 | 28.6 (B 1, L 300) -- see below
  path_plan: 0.9 .. 1.0 | 0.9 .. 1.0, t = 0 and t = 1 included
  masked_mse: random mask <= 3.4 | 3.3 (per_sample 27720), all ones <= 5.5 | 6.1 (per_sample 2047, where the floor happens to be
      1e-8; the device's error is 5.7e-8), a single 1 at the last element: that element's fp32 (p - t)^2 exactly at all 11 sizes
No case needed a change to a kernel or a launcher; every exact assertion held, every guard was untouched, and a second call gave
the same bits.

The one ratio near the factor, the torsions at 100 A, is a difference of formula, not of rounding: k_atom14_to_cond follows the
reference's own sequence, `torsion_frames.invert().apply(p)` = R^T p + (-(R^T t)) (geometry.py:178), whose two terms are of the
size of the coordinates and cancel down to a bond length, while the oracle's rigid_invert_apply subtracts first, R^T (p - t).  The
kernel's error there is 3.8e-5 of a unit (sin, cos) pair at worst, the fp32 oracle's 2.1e-6; at centre 0 the two agree to 2.2 x.
"""
from __future__ import annotations

import functools
import math

import torch

from ipa_ref import FACTOR, ULPS, _rows, check, report_line   # noqa: F401  (check / report_line: re-exported to the test modules)
from oracle import mdgen_oracle as O

GUARD = 64          # elements behind every device output that no kernel may touch
PI_FAMILIES = ("pi", "pi-1e-07", "pi-0.0001", "pi-0.01")


# ---- small helpers ------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(gen, *shape):
    x = torch.randn(*shape, generator=gen, dtype=torch.float64)
    return x / x.norm(dim=-1, keepdim=True)


def _rand_rots(gen, *shape):
    """Random rotations: fp64 quat_to_rot of unit quaternions, rounded to fp32."""
    return O.quat_to_rot(_unit(gen, *shape, 4)).float().contiguous()


def _spread_norms(gen, shape, lo, hi):
    """10^U(lo, hi), fp64."""
    return 10.0 ** (lo + (hi - lo) * torch.rand(*shape, generator=gen, dtype=torch.float64))


def _to(dtype, inp, *keys):
    return [inp[k].to(dtype) for k in keys]


def w_nonneg(q):
    return torch.where(q[..., :1] < 0, -q, q)


def _all(x):
    return torch.ones(x.shape[0], dtype=torch.bool)


def _vec(dev, ref, k):
    """Row metric over every row of the last dimension(s) flattened to k."""
    d, r = dev.reshape(-1, k), ref.reshape(-1, k)
    return _rows(d, r, _all(r), _all(r))


def _quat(dev, ref, gate):
    """((max, rel-L2) of the quaternion rows, the rows that took the sign-free path).  gate None: every row sign-free (the
    floor: eigh's sign is arbitrary); else rows with |w_ref| > gate are compared with their sign."""
    d, r = dev.reshape(-1, 4).double(), w_nonneg(ref.reshape(-1, 4).double())
    free = torch.ones(r.shape[0], dtype=torch.bool) if gate is None else r[:, 0].abs() <= gate
    e = (d - r).norm(dim=-1)
    e = torch.where(free, torch.minimum(e, (d + r).norm(dim=-1)), e)
    return (float(e.max()), float(e.norm() / r.norm())), free        # unit rows: the scale of _rows is 1


# ---- the cases ----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, group, **p):
        self.group, self.p = group, p
        self.id = group + "-" + "-".join(f"{k}{v}" for k, v in p.items())
        self.seed = 9000 + sum(ord(c) * (i + 1) for i, c in enumerate(self.id)) % 100000

    def __getattr__(self, k):
        try:
            return self.p[k]
        except KeyError:
            raise AttributeError(k) from None

    def __hash__(self):
        return hash(self.id)

    def __eq__(self, o):
        return isinstance(o, Case) and o.id == self.id


R2Q_FAMILIES = ("random",) + PI_FAMILIES + ("small", "dom_w", "dom_x", "dom_y", "dom_z", "relative")
MSE_SIZES = (1, 255, 256, 257, 1792, 1793, 2047, 2048, 2049, 4113, 27720)
MSE_MASKS = ("random", "ones", "last")

CASES = (
    # the 256-thread launch edge of every one-thread-per-frame kernel
    [Case("algebra", n=n) for n in (1, 255, 256, 257, 513)]
    # k_rigid_apply's i / ppf: a block boundary at a frame boundary (ppf 1), inside frame 18 (256 = 18 * 14 + 4), inside frame 6
    + [Case("apply", n=n, ppf=ppf) for n, ppf in ((257, 1), (19, 14), (7, 37))]
    + [Case("r2q", family=f) for f in R2Q_FAMILIES]
    + [Case("prep", B=B, T=T, L=L, tps=tps, ci=ci if isinstance(ci, int) else T + ci[1])
       for B, T, L in ((2, 5, 3), (1, 1, 4), (3, 7, 37)) for tps in (0, 1) for ci in (0, 1, 3, ("T", 0), ("T", 5))]
    + [Case("post", B=B, T=T, L=L, tps=tps) for B, T, L in ((2, 3, 23), (1, 13, 20)) for tps in (0, 1)]
    + [Case("cond", B=B, L=L, centre=c) for B, L in ((3, 23), (1, 300)) for c in (0, 100)]
    + [Case("plan", gvp=g, per=per) for g in (0, 1) for per in (1, 255, 257, 630)]
    + [Case("mse", per=per) for per in MSE_SIZES]
)
CASES = list({c.id: c for c in CASES}.values())     # (T = 1: cond_interval 1 is also T)
PLAN_T = (0.0, 1e-4, 0.5, 1 - 1e-4, 1.0)


# ---- algebra: compose, invert, apply, quat_to_rot, from_3_points, rot_to_quat at one n -----------------------------------------
def _bonded(gen, n):
    """Three bonded atoms per frame, 1.5 A apart, bond angle 60 .. 120 degrees, around 100 A; the LAST frame's three points
    coincide (the reference's eps keeps that finite: R = 0)."""
    org = 100 + 10 * torch.randn(n, 3, generator=gen, dtype=torch.float64)
    u = _unit(gen, n, 3)
    v = _unit(gen, n, 3)
    v = v - u * (u * v).sum(-1, keepdim=True)
    v = v / v.norm(dim=-1, keepdim=True)
    th = 1.05 + 1.05 * torch.rand(n, 1, generator=gen, dtype=torch.float64)
    a, b = org + 1.5 * u, org + 1.5 * (torch.cos(th) * u + torch.sin(th) * v)
    a[-1], b[-1] = org[-1], org[-1]
    return a.float(), org.float(), b.float()


def _algebra_inputs(c):
    g = _gen(c.seed)
    n = c.n
    a, o, b = _bonded(g, n)
    return dict(R1=_rand_rots(g, n), R2=_rand_rots(g, n), t1=100 * torch.randn(n, 3, generator=g), t2=100 * torch.randn(n, 3, generator=g),
                p=100 * torch.randn(n, 3, generator=g), q=(_unit(g, n, 4) * _spread_norms(g, (n, 1), -3, 3)).float(), p3a=a, p3b=o, p3c=b)


def _algebra_oracle(c, inp, dt):
    R1, R2, t1, t2, p, q, a, o, b = _to(dt, inp, "R1", "R2", "t1", "t2", "p", "q", "p3a", "p3b", "p3c")
    out = {}
    out["comp_R"], out["comp_t"] = O.rigid_compose(R1, t1, R2, t2)
    out["inv_R"], out["inv_t"] = O.rigid_invert(R1, t1)
    out["apply"], out["inv_apply"] = O.rigid_apply(R1, t1, p), O.rigid_invert_apply(R1, t1, p)
    out["q2r_raw"] = O.quat_to_rot(q)
    out["q2r_norm"] = O.from_tensor_7(torch.cat([q, torch.zeros_like(q[:, :3])], -1), normalize_quats=True)[0]
    out["f3_R"], out["f3_t"] = O.from_3_points(a, o, b)
    out["quat"] = w_nonneg(O.rot_to_quat(R1))
    out["ident_t"] = O.rigid_compose(R1, t1, out["inv_R"], out["inv_t"])[1]     # A o A^-1: zero up to 1e-7 |t|
    return out


_ALGEBRA_ROWS = dict(comp_R=9, comp_t=3, inv_R=9, inv_t=3, apply=3, inv_apply=3, q2r_raw=9, q2r_norm=9, f3_R=9, f3_t=3)


def _ident(t, inp):
    """|t of A o A^-1| against the size of A's translations.  (The exact value is not a reference to measure against: it is what
    the fp32 rotation lacks of being orthogonal, 1e-7 of |t|, and nothing else.)"""
    e = t.double().norm(dim=-1)
    s = float(inp["t1"].double().norm(dim=-1).pow(2).mean().sqrt())
    return float(e.max() / s), float(e.norm() / (s * math.sqrt(e.numel())))


def _algebra_measure(c, inp, out, ref, gate):
    m = {k: _vec(out[k], ref[k], r) for k, r in _ALGEBRA_ROWS.items()}
    m["quat"], free = _quat(out["quat"], ref["quat"], None if gate is None else gate["quat"][0])
    m["ident_t"] = _ident(out["ident_t"], inp)
    return m, free


def _algebra_exact(c, inp, out, ref, gate):
    assert torch.equal(out["inv_R"], inp["R1"].transpose(-1, -2)), "rigid_invert: the rotation is not the bit-exact transpose"
    # three coincident points (the last frame): R exactly 0, t the origin, nothing but finite values
    assert bool((out["f3_R"][-1] == 0).all()) and torch.equal(out["f3_t"][-1], inp["p3b"][-1]), "from_3_points: coincident points"
    _quat_exact(out["quat"], gate["quat"][0])


def _quat_exact(q, gate):
    assert bool((q[..., 0] >= 0).all()), "quaternion with w < 0"
    assert float((q.double().norm(dim=-1) - 1).abs().max()) <= gate, "quaternion not of unit norm"


# ---- apply: (n, ppf) -----------------------------------------------------------------------------------------------------------
def _apply_inputs(c):
    g = _gen(c.seed)
    return dict(R=_rand_rots(g, c.n), t=100 * torch.randn(c.n, 3, generator=g), p=100 * torch.randn(c.n, c.ppf, 3, generator=g))


def _apply_oracle(c, inp, dt, frame_of=None):
    """frame_of (tests only, fault injection): the frame index of every flat point."""
    R, t, p = _to(dt, inp, "R", "t", "p")
    if frame_of is not None:
        f = frame_of(c.n, c.ppf).view(c.n, c.ppf)
        R, t = R[f], t[f]
    else:
        R, t = R[:, None], t[:, None]
    return dict(apply=O.rigid_apply(R, t, p), inv_apply=O.rigid_invert_apply(R, t, p))


def _apply_measure(c, inp, out, ref, gate):
    return {k: _vec(out[k], ref[k], 3) for k in ("apply", "inv_apply")}, None


# ---- rot_to_quat families ------------------------------------------------------------------------------------------------------
def _axis_angle(axis, ang):
    return torch.cat([torch.cos(ang / 2), torch.sin(ang / 2) * axis], -1)


def _r2q_inputs(c, n=257):
    g = _gen(c.seed)
    f = c.family
    if f == "relative":      # what frame_offset7 / k_rel7 feed rot2quat: R1^T R2 formed in fp32, orthogonal to 1e-7 only
        R1, R2 = _rand_rots(g, n), _rand_rots(g, n)
        return dict(R=torch.einsum("nji,njk->nik", R1, R2).contiguous())
    if f == "random":
        q = _unit(g, n, 4)
    elif f in PI_FAMILIES:
        axis = _unit(g, n, 3)
        eye = torch.eye(3, dtype=torch.float64)
        axis[:6] = torch.cat([eye, -eye])          # about +-x, +-y, +-z
        delta = 0.0 if f == "pi" else float(f[3:])
        q = _axis_angle(axis, torch.full((n, 1), math.pi - delta, dtype=torch.float64))
        if f == "pi":
            q[:, 0] = 0.0                          # cos(pi / 2) exactly
    elif f == "small":
        ang = 1e-4 * torch.rand(n, 1, generator=g, dtype=torch.float64)
        ang[0] = 0.0                               # the identity itself
        q = _axis_angle(_unit(g, n, 3), ang)
    else:                                          # dom_w .. dom_z: that component the largest in magnitude, either sign
        k = "wxyz".index(f[-1])
        q = _unit(g, n, 4)
        big = q.abs().argmax(-1)
        idx = torch.arange(n)
        qk, qb = q[idx, k].clone(), q[idx, big].clone()
        q[idx, big], q[idx, k] = qk, qb
        assert bool((q.abs().argmax(-1) == k).all())
    return dict(R=O.quat_to_rot(q).float().contiguous())


def _r2q_oracle(c, inp, dt):
    return dict(quat=w_nonneg(O.rot_to_quat(inp["R"].to(dt))))


def _r2q_measure(c, inp, out, ref, gate):
    m, free = _quat(out["quat"], ref["quat"], None if gate is None else gate["quat"][0])
    return {"quat": m}, free


def _r2q_exact(c, inp, out, ref, gate):
    _quat_exact(out["quat"], gate["quat"][0])


# ---- prep_latents --------------------------------------------------------------------------------------------------------------
def _pi_frame(c):
    """The frame that is turned by pi relative to frame 0 (None at T = 1); never T - 1 when T >= 3."""
    return None if c.T == 1 else 1


def _prep_inputs(c):
    g = _gen(c.seed)
    B, T, L = c.B, c.T, c.L
    R = O.quat_to_rot(_unit(g, B, T, L, 4))
    if _pi_frame(c) is not None:
        q = torch.cat([torch.zeros(B, L, 1, dtype=torch.float64), _unit(g, B, L, 3)], -1)
        R[:, _pi_frame(c)] = O.rot_matmul(R[:, 0], O.quat_to_rot(q))
    return dict(rots=R.float().contiguous(), trans=100 + 10 * torch.randn(B, T, L, 3, generator=g),
                torsions=torch.randn(B, T, L, 7, 2, generator=g), seqres=torch.zeros(B, L, dtype=torch.long))


def _prep_oracle(c, inp, dt):
    B, L = c.B, c.L
    batch = dict(inp, mask=torch.ones(B, L), torsion_mask=torch.ones(B, L, 7))
    cfg = dict(sim_condition=not c.tps, tps_condition=bool(c.tps), cond_interval=c.ci,
               compute_dtype="float64" if dt == torch.float64 else "float32")
    prep = O.prep_batch(batch, cfg)
    kw = prep["model_kwargs"]
    return dict(latents=prep["latents"], x_cond=kw["x_cond"], x_cond_mask=kw["x_cond_mask"])


def _prep_measure(c, inp, out, ref, gate):
    lat, rl = out["latents"], ref["latents"]
    m, free = {}, []
    for r in range(2 if c.tps else 1):
        q = f"quat{r}"
        m[q], fr = _quat(lat[..., 7 * r:7 * r + 4], rl[..., 7 * r:7 * r + 4], None if gate is None else gate[q][0])
        free.append(fr.view(c.B, c.T, c.L))
        m[f"trans{r}"] = _vec(lat[..., 7 * r + 4:7 * r + 7], rl[..., 7 * r + 4:7 * r + 7], 3)
    return m, free


def _prep_exact(c, inp, out, ref, gate):
    lat, xc, cm = out["latents"], out["x_cond"], out["x_cond_mask"]
    D = 28 if c.tps else 21
    assert lat.shape[-1] == D
    assert torch.equal(cm, ref["x_cond_mask"]), "x_cond_mask differs from the oracle's"
    want = torch.where(cm[..., None] == 1, lat, torch.zeros_like(lat))
    assert torch.equal(xc.view(torch.int32), want.view(torch.int32)), "x_cond is not (latents where the mask is 1, +0.0 elsewhere), bit for bit"
    assert bool((lat[:, 0, :, 4:7] == 0).all()), "translation offset of frame 0 to itself is not exactly 0"
    if c.tps:
        assert bool((lat[:, -1, :, 11:14] == 0).all()), "translation offset of frame T - 1 to itself is not exactly 0"
    assert torch.equal(lat[..., D - 14:].view(torch.int32), inp["torsions"].reshape(c.B, c.T, c.L, 14).view(torch.int32)), "torsion columns"
    for r in range(2 if c.tps else 1):
        _quat_exact(lat[..., 7 * r:7 * r + 4], gate[f"quat{r}"][0])


# ---- samples_to_atom14 ---------------------------------------------------------------------------------------------------------
def _seqres(B, L):
    """Every residue type cycled; L = 23 holds 0 .. 20, L = 20 holds 1 .. 20; each sample starts 7 types further on."""
    first = 0 if L >= 21 else 1
    return torch.stack([(torch.arange(L) + first + 7 * b) % 21 for b in range(B)])


def _post_inputs(c):
    g = _gen(c.seed)
    B, T, L, D = c.B, c.T, c.L, 28 if c.tps else 21
    s = torch.randn(B, T, L, D, generator=g, dtype=torch.float64)        # TPS: columns 7 .. 13 are the second offset, unused
    s[..., :4] = _unit(g, B, T, L, 4) * _spread_norms(g, (B, T, L, 1), -2, 2)
    s[..., 4:7] = 3 * torch.randn(B, T, L, 3, generator=g, dtype=torch.float64)
    tors = _unit(g, B, T, L, 7, 2) * _spread_norms(g, (B, T, L, 7, 1), -2, 2)
    s[..., D - 14:] = tors.reshape(B, T, L, 14)
    return dict(samples=s.float().contiguous(), rot0=_rand_rots(g, B, L), trans0=100 + 10 * torch.randn(B, L, 3, generator=g),
                seqres=_seqres(B, L))


def _post_oracle(c, inp, dt, tps=None, rot0=None):
    """tps / rot0 (tests only, fault injection): the flag and the start rotations the post-processing is run with."""
    s, r0, t0 = _to(dt, inp, "samples", "rot0", "trans0")
    r0 = r0 if rot0 is None else rot0(r0)
    a14, _ = O.postprocess(s, (r0[:, None], t0[:, None]), inp["seqres"], dict(tps_condition=bool(c.tps if tps is None else tps)))
    return dict(atom14=a14)


def _post_measure(c, inp, out, ref, gate):
    return {"atom14": _vec(out["atom14"], ref["atom14"], 3)}, None


def _post_exact(c, inp, out, ref, gate):
    m = O.tables()["atom14_mask"][inp["seqres"]][:, None].expand(c.B, c.T, c.L, 14)
    assert bool((out["atom14"][m == 0] == 0).all()), "an atom with atom14_mask 0 is not exactly 0"


# ---- atom14_to_cond ------------------------------------------------------------------------------------------------------------
def _cond_inputs(c):
    """atom14 = the fp64 frames_torsions_to_atom14 of random frames on a 3.8 A chain and random torsions, rounded to fp32."""
    g = _gen(c.seed)
    B, L = c.B, c.L
    sq = _seqres(B, L) if L < 30 else (torch.arange(L) % 21)[None].expand(B, L).contiguous()
    R = O.quat_to_rot(_unit(g, B, L, 4))
    t = float(c.centre) + torch.cumsum(3.8 * _unit(g, B, L, 3), 1)
    t = t - t.mean(1, keepdim=True) + float(c.centre)
    a14 = O.frames_torsions_to_atom14(R, t, _unit(g, B, L, 7, 2), sq)
    return dict(atom14=a14.float().contiguous(), seqres=sq)


def _cond_oracle(c, inp, dt, view=None):
    """view (tests only, fault injection): the (B, L) the chain is cut into before the torsions are taken."""
    a, sq = inp["atom14"].to(dt), inp["seqres"]
    if view is not None:
        a, sq = a.reshape(*view, 14, 3), sq.reshape(*view)
    glue = O.rollout_glue(a, sq)
    _, tm = O.atom37_to_torsions(O.atom14_to_atom37(a, sq), sq)
    sh = (c.B, c.L)
    return dict(rots=glue["rots"][:, 0].reshape(*sh, 3, 3), trans=glue["trans"][:, 0].reshape(*sh, 3),
                torsions=glue["torsions"][:, 0].reshape(*sh, 7, 2), torsion_mask=tm.reshape(*sh, 7).to(dt))


def _cond_measure(c, inp, out, ref, gate):
    m = {"rots": _vec(out["rots"], ref["rots"], 9), "trans": _vec(out["trans"], ref["trans"], 3)}
    valid = ref["torsion_mask"].reshape(-1) == 1
    m["torsions"] = _rows(out["torsions"].reshape(-1, 2), ref["torsions"].reshape(-1, 2), valid, valid)
    return m, None


def _cond_exact(c, inp, out, ref, gate):
    tm = out["torsion_mask"]
    assert torch.equal(tm.double(), ref["torsion_mask"].double()), "torsion_mask differs from the oracle's"
    assert bool((tm[:, 0, :2] == 0).all()), "pre-omega / phi of residue 0 not masked: the previous sample's last residue was read"
    masked = out["torsions"].reshape(-1, 2)[ref["torsion_mask"].reshape(-1) != 1].double()
    assert len(masked) and float(masked.norm(dim=-1).max()) <= 1 + gate["torsions"][0], "a masked torsion pair of norm > 1"


def _cond_conditions(c, ref):
    tm = ref["torsion_mask"].reshape(-1, 7)
    per_kind = (tm == 1).sum(0)
    assert int(per_kind.min()) >= 4, (c.id, per_kind.tolist())
    assert float((tm == 1).double().mean()) >= 0.6, (c.id, float((tm == 1).double().mean()))


# ---- path_plan -----------------------------------------------------------------------------------------------------------------
def _plan_inputs(c):
    g = _gen(c.seed)
    B = len(PLAN_T)
    return dict(t=torch.tensor(PLAN_T, dtype=torch.float32), x0=torch.randn(B, c.per, generator=g), x1=torch.randn(B, c.per, generator=g))


def _plan_oracle(c, inp, dt, t_of=None):
    t, x0, x1 = _to(dt, inp, "t", "x0", "x1")
    xt, ut = O.path_plan(t if t_of is None else t_of(t), x0, x1, "GVP" if c.gvp else "Linear")
    return dict(xt=xt, ut=ut)


def _plan_measure(c, inp, out, ref, gate):
    return {k: _vec(out[k], ref[k], c.per) for k in ("xt", "ut")}, None


# ---- masked_mse ----------------------------------------------------------------------------------------------------------------
MSE_B = 3


def _mse_inputs(c):
    g = _gen(c.seed)
    inp = dict(pred=torch.randn(MSE_B, c.per, generator=g), target=torch.randn(MSE_B, c.per, generator=g))
    rnd = (torch.rand(MSE_B, c.per, generator=g) < 0.7).float()
    rnd[:, 0] = 1                                  # (never an empty mask)
    last = torch.zeros(MSE_B, c.per)
    last[:, -1] = 1
    inp.update(mask_random=rnd, mask_ones=torch.ones(MSE_B, c.per), mask_last=last)
    return inp


def _mse_oracle(c, inp, dt, loss_of=None):
    p, t = _to(dt, inp, "pred", "target")
    f = loss_of or O.mean_flat
    return {f"loss_{k}": f((p - t) ** 2, inp[f"mask_{k}"].to(dt)) for k in MSE_MASKS}


def _mse_measure(c, inp, out, ref, gate):
    return {k: _vec(out[k], ref[k], 1) for k in ref}, None


def _mse_exact(c, inp, out, ref, gate):
    d = inp["pred"][:, -1] - inp["target"][:, -1]
    assert torch.equal(out["loss_last"].float(), d * d), "a single 1 at the last element: the loss is not that element's fp32 (p - t)^2"


# ---- reference, gate, verification ----------------------------------------------------------------------------------------------
_G = {
    "algebra": (_algebra_inputs, _algebra_oracle, _algebra_measure, _algebra_exact),
    "apply": (_apply_inputs, _apply_oracle, _apply_measure, None),
    "r2q": (_r2q_inputs, _r2q_oracle, _r2q_measure, _r2q_exact),
    "prep": (_prep_inputs, _prep_oracle, _prep_measure, _prep_exact),
    "post": (_post_inputs, _post_oracle, _post_measure, _post_exact),
    "cond": (_cond_inputs, _cond_oracle, _cond_measure, _cond_exact),
    "plan": (_plan_inputs, _plan_oracle, _plan_measure, None),
    "mse": (_mse_inputs, _mse_oracle, _mse_measure, _mse_exact),
}


def oracle(case, inp, dtype, **fault):
    return _G[case.group][1](case, inp, dtype, **fault)


def _sign_free_allowed(case, free):
    """Assert that only the rows that may take the sign-free quaternion path do: none outside the pi families / the frame of
    prep_latents that is turned by pi against frame 0 (its first quaternion)."""
    if free is None:
        return
    if case.group == "prep":
        ok = torch.zeros(case.B, case.T, case.L, dtype=torch.bool)
        if _pi_frame(case) is not None:
            ok[:, _pi_frame(case)] = True
        assert not bool((free[0] & ~ok).any()), (case.id, "sign-free rows off the pi frame")
        assert all(not bool(f.any()) for f in free[1:]), (case.id, "sign-free rows in the second quaternion")
    elif not (case.group == "r2q" and case.family in PI_FAMILIES):
        assert not bool(free.any()), (case.id, "sign-free rows", int(free.sum()))


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, fp64 outputs, {quantity: (gate of max, gate of rel)}, {quantity: floors}) of a case; computed once, shared, never
    modified.  Asserts the conditions of the case table: the sign-free rule and the torsion shares."""
    inputs, orc, measure, _ = _G[case.group]
    inp = inputs(case)
    ref = orc(case, inp, torch.float64)
    floor, _ = measure(case, inp, standin(case, inp), ref, None)
    gate = {k: tuple(max(FACTOR * f, ULPS) for f in v) for k, v in floor.items()}
    _, free = measure(case, inp, ref, ref, gate)
    _sign_free_allowed(case, free)
    if case.group == "cond":
        _cond_conditions(case, ref)
    return inp, ref, gate, floor


def standin(case, inp, **fault):
    """The oracle in torch fp32 on the CPU: what the floors are measured on, and the stand-in device of the CPU tests."""
    return {k: (v if v.dtype == torch.long else v.float()) for k, v in oracle(case, inp, torch.float32, **fault).items()}


def verify(case, out, exact=True):
    """`out` (a dict like the oracle's, CPU tensors) against the case's gates and exact assertions -> (metrics, floors).
    Raises AssertionError.  Non-finite values fail: every comparison is written so that a NaN is a miss."""
    inp, ref, gate, floor = reference(case)
    _, _, measure, ex = _G[case.group]
    for k, v in out.items():
        assert v.shape == ref[k].shape, (case.id, k, v.shape, ref[k].shape)
        assert v.dtype == torch.long or bool(torch.isfinite(v).all()), (case.id, k, "non-finite values")
    got, _ = measure(case, inp, out, ref, gate)
    check(case.id, got, gate)
    if exact and ex is not None:
        ex(case, inp, out, ref, gate)
    return got, floor
