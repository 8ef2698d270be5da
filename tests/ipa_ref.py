"""The invariant point attention core (mdgen/model/ipa.py:126-254 with c_z = 0, between the four input projections and
linear_out) restated in plain torch, in the layouts of the HIP kernels (csrc/common.h kIpaProj / kIpaFeat); the inputs, the case
table, the row metric and the floor-relative gate of tests/test_ipa_attention_{cpu,gpu}.py.

A test helper, not a test module.  `core` is pinned to the oracle (and so to the reference's goldens) by
test_ipa_attention_cpu.py; the device is compared with `core` in fp64 on the device's own fp32 inputs.

The gate is not a fixed number.  For every case and quantity, `floor` is the metric of `core` run in torch fp32 on the CPU
against `core` in fp64, and gate = max(32 * floor, 32 * 2^-24): 32 x for what the kernels legitimately do differently from
torch's fp32 (online softmax renormalised per 32-key tile, the slice merge, another expf, FMA contraction), 32 fp32 ulps for
floors that happen to be tiny.  Floors on valid rows: compact 1e-7 .. 6e-7 (feat, dproj), 5e-8 (lse), up to 1.4e-6 (dhead_w);
chain 1e-6 .. 2e-5.  Padded QUERY rows have a floor of about 1.7e-3: 1e5 (m_i m_j - 1) leaves all their logits near -1e5, where
an fp32 ulp is 0.008, so every weight of such a row carries a relative error of that size -- in torch's fp32 as in the kernels,
which is why those rows get a floor of their own.

Worst measured device / floor ratio per quantity over the cases of CASES (row max | rel-L2), MI355X:
  feat 1.9 | 1.3 (B 1, L 257, cut scratch | B 1, L 32)     feat on padded query rows 1.0 | 1.0     lse 1.6 | 1.6 (L 32 | L 257)
  dproj 11.7 | 7.3 (B 1, L 5; 5.0 | 3.2 beyond L = 5)       dhead_w 8.9 | 9.6 (B 6, L 100)
against the factor 32.  L = 1: d head_w is exactly zero in the reference (see `metrics`); the device leaves 4.2e-10 of the scale
used there, gate 1.9e-6.  No case needed a change to a kernel or a launcher.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

PART_FULL = 16 << 20           # floats: the training step's split scratch (csrc/train.inc kPartFloats)
FWD_REC, BWD_ROW = 4 * 58, 676  # floats per token and slice of the forward / backward scratch (kIpaFwdRec, kIpaPartRow)
HEAD_W = (-2.0, 0.0, 0.5413, 25.0)   # head 3: softplus on its linear branch (> 20), forward and backward
FACTOR, ULPS = 32.0, 32.0 * 2.0 ** -24


# ---- the reference ------------------------------------------------------------------------------------------------------------
def core(proj, rot, trans, mask, head_w, hooks=None):
    """proj [G L][672] (q 128 | kv 256 | q_points 96 | kv_points 192), rot [B][L][3][3], trans [B][L][3], mask [B][L],
    head_w [4] -> features [G L][256] (o 128 | o_pt x | y | z | norm, 32 each), log-sum-exp of the logits [G L][4].  Group g
    uses the frames and the mask of sample g % B.  dtype follows the inputs; differentiable; one head at a time ([G][L][L][8][3]
    is the largest intermediate).  hooks (tests only, fault injection on a stand-in): "logits"(raw, mask_term, h) -> logits,
    "softplus"(w), "frames"(G, B) -> sample of every group, "probs"(a, h): observer of the attention weights."""
    hooks = hooks or {}
    B, L = mask.shape
    G = proj.shape[0] // L
    fi = hooks["frames"](G, B) if "frames" in hooks else torch.arange(G) % B
    R, t, m = rot[fi], trans[fi], mask[fi]
    p = proj.view(G, L, 672)

    def to_global(cols, n):      # [x-block | y-block | z-block] of n points -> R p + t   (ipa.py:126-151)
        x = torch.stack(torch.split(cols, n, dim=-1), dim=-1)                    # [G, L, n, 3]
        return torch.einsum("glab,glnb->glna", R, x) + t[:, :, None]

    q = p[..., 0:128].view(G, L, 4, 32)
    kv = p[..., 128:384].view(G, L, 4, 64)
    qp = to_global(p[..., 384:480], 32).view(G, L, 4, 8, 3)
    kvp = to_global(p[..., 480:672], 64).view(G, L, 4, 16, 3)
    hw = hooks.get("softplus", F.softplus)(head_w) * math.sqrt(1.0 / (3 * (8 * 9.0 / 2)))     # :176-181
    mterm = 1e5 * (m[:, :, None] * m[:, None, :] - 1)                                         # :188-190
    o, op, lse = [], [], []
    for h in range(4):
        k, v = kv[:, :, h, :32], kv[:, :, h, 32:]
        kp, vp = kvp[:, :, h, :8], kvp[:, :, h, 8:]
        raw = torch.einsum("gic,gjc->gij", q[:, :, h], k) * math.sqrt(1.0 / (3 * 32))          # :161-168
        d2 = ((qp[:, :, None, h] - kp[:, None]) ** 2).sum(-1)                                  # [G, i, j, 8]  :171-175
        raw = raw + (d2 * hw[h]).sum(-1) * (-0.5)                                              # :182-185
        lg = hooks["logits"](raw, mterm, h) if "logits" in hooks else raw + mterm
        a = torch.softmax(lg, dim=-1)                                                          # :203
        if "probs" in hooks:
            hooks["probs"](a, h)
        lse.append(torch.logsumexp(lg, dim=-1))
        o.append(torch.einsum("gij,gjc->gic", a, v))                                           # :209-212
        g = torch.einsum("gij,gjpx->gipx", a, vp) - t[:, :, None]                              # :216-226
        op.append(torch.einsum("glba,glpb->glpa", R, g))                                       # R^T (p - t)
    o = torch.stack(o, 2).reshape(G, L, 128)
    op = torch.stack(op, 2).reshape(G, L, 32, 3)
    opn = torch.sqrt((op ** 2).sum(-1) + 1e-8)                                                 # :229-231
    feat = torch.cat([o, op[..., 0], op[..., 1], op[..., 2], opn], dim=-1)                     # :250-254
    return feat.reshape(G * L, 256), torch.stack(lse, -1).reshape(G * L, 4)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def inputs(B, ngroups, L, kind, seed):
    """fp32 inputs of one case.  "compact": translations 0.5 randn, point columns scaled by 0.3 -- attention spread over many
    keys, so a wrong or missing key moves the output; "chain": translations cumsum(2.2 randn), unit points -- protein-like
    distances, peaked softmax, strongly cancelling logits.  Mask: 20 % random padding in every sample, the last max(1, L // 3)
    residues of the last sample padded as well (L >= 96: a whole 32-key tile), with B >= 3 sample 1 keeps a single real
    residue; a sample left with no real residue gets residue 0 back.  dfeat: randn, zero on padded query rows."""
    from oracle import mdgen_oracle as O
    assert kind in ("compact", "chain") and ngroups % B == 0
    gen = torch.Generator().manual_seed(seed)
    M = ngroups * L
    proj = torch.randn(M, 672, generator=gen)
    quat = torch.randn(B, L, 4, generator=gen)
    rot = O.quat_to_rot(quat / quat.norm(dim=-1, keepdim=True)).contiguous()
    step = torch.randn(B, L, 3, generator=gen)
    if kind == "compact":
        trans = 0.5 * step
        proj[:, 384:] *= 0.3
    else:
        trans = torch.cumsum(2.2 * step, 1)
    mask = (torch.rand(B, L, generator=gen) > 0.2).float()
    mask[B - 1, L - max(1, L // 3):] = 0
    if B >= 3:
        keep = int(torch.randint(0, L, (1,), generator=gen))
        mask[1] = 0
        mask[1, keep] = 1
    for b in range(B):
        if mask[b].sum() == 0:
            mask[b, 0] = 1
    qmask = mask[torch.arange(ngroups) % B].reshape(M)
    dfeat = torch.randn(M, 256, generator=gen) * qmask[:, None]
    dhw0 = torch.randn(4, generator=gen)          # dhead_w is accumulated into: what it holds before the call
    return dict(proj=proj, rot=rot, trans=trans.contiguous(), mask=mask, head_w=torch.tensor(HEAD_W), dfeat=dfeat, qmask=qmask,
                dhw0=dhw0)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
class Case:
    """scratch: "full" (the training step's 16 Mi floats), a float count, or None (part = NULL).  fwd / bwd: (slices launched,
    of them empty) as the comment of the table claims them; tiled: the forward kernel.  bwd None: forward only."""

    def __init__(self, ngroups, B, L, kind, scratch, tiled, fwd, bwd):
        self.ngroups, self.B, self.L, self.kind, self.scratch = ngroups, B, L, kind, scratch
        self.tiled, self.fwd, self.bwd = tiled, fwd, bwd
        self.seed = 7000 + 31 * L + B + 1000 * ngroups
        s = {"full": "", None: "-nopart"}.get(scratch, f"-part{scratch}")
        self.id = f"g{ngroups}b{B}L{L}-{kind}{s}"

    @property
    def part_floats(self):
        return PART_FULL if self.scratch == "full" else (self.scratch or 0)


def _c(B, L, tiled, fwd, bwd, kind="compact", scratch="full", ngroups=None):
    return Case(ngroups or B, B, L, kind, scratch, tiled, fwd, bwd)


_M257 = 257
CASES = [
    # one thread per (query, head); the backward always runs the tiled kernels (one tile: one slice)
    _c(2, 1, False, (1, 0), (1, 0)), _c(1, 5, False, (1, 0), (1, 0)), _c(2, 23, False, (1, 0), (1, 0)),
    # LDS-tiled, one 32-key tile: one slice; two and three tiles: one tile per slice
    _c(1, 24, True, (1, 0), (1, 0)), _c(2, 31, True, (1, 0), (1, 0)), _c(1, 32, True, (1, 0), (1, 0)),
    _c(2, 33, True, (2, 0), (2, 0)), _c(1, 64, True, (2, 0), (2, 0)), _c(2, 65, True, (3, 0), (3, 0)),
    # the 256-query edge: eight tiles in eight slices; from 257 two query tiles per (group, head), nine / ten key tiles in
    # slices of three / two whole tiles -- B 2, L 257: 4 slices, the last past L; B 1, L 300: 8 slices, 3 past L
    _c(2, 255, True, (8, 0), (8, 0)), _c(1, 256, True, (8, 0), (8, 0)), _c(2, 257, True, (4, 1), (4, 1)),
    _c(1, 300, True, (8, 3), (8, 3)),
    # empty slices: 5 tiles in 4 slices of 2; 7 tiles in 6 slices of 2; 4 tiles in 3 slices of 2
    _c(4, 130, True, (4, 1), (4, 1)), _c(4, 130, True, (4, 1), (4, 1), kind="chain"),
    _c(3, 200, True, (6, 2), (6, 2)), _c(3, 200, True, (6, 2), (6, 2), kind="chain"),
    _c(6, 100, True, (3, 1), (3, 1)), _c(6, 100, True, (3, 1), (3, 1), kind="chain"),
    # scratch limits at B 1, L 257 (full scratch: 8 slices of 2 tiles, 3 empty, both directions): exactly four backward
    # slices' floats (forward uncut); exactly five forward slices' (backward: one); one float short of two forward slices'; NULL
    _c(1, 257, True, (8, 3), (4, 1), scratch=4 * _M257 * BWD_ROW),
    _c(1, 257, True, (5, 0), (1, 0), scratch=5 * _M257 * FWD_REC),
    _c(1, 257, True, (1, 0), (1, 0), scratch=2 * _M257 * FWD_REC - 1),
    _c(1, 257, True, (1, 0), (1, 0), scratch=None),
    # the sampler's call, forward only: ngroups = steps * B, frames of group g = sample g % B; + the bf16 feature rows
    _c(2, 33, True, (2, 0), None, ngroups=6), _c(1, 257, True, (2, 0), None, ngroups=4),
]


# ---- the metric and the gate --------------------------------------------------------------------------------------------------
def _rows(dev, ref, sel, scale_sel):
    """(max over the rows `sel` of |dev - ref| / rms over the rows `scale_sel` of |ref|, rel-L2 of the rows `sel`)."""
    dev, ref = dev.double(), ref.double()
    scale = float(ref[scale_sel].norm(dim=-1).pow(2).mean().sqrt().clamp_min(1e-300))
    if not bool(sel.any()):
        return 0.0, 0.0
    e = (dev[sel] - ref[sel]).norm(dim=-1)
    return float(e.max() / scale), float(e.norm() / ref[sel].norm().clamp_min(1e-300))


def metrics(dev, ref, inp):
    """{quantity: (max row error, rel-L2)} of the outputs `dev` against `ref` (dicts of feat, lse and, with a backward, dproj,
    dhead_w = the gradient alone) on the inputs `inp`.  feat: valid query rows; feat_pad: padded query rows (scaled by the valid
    rows); lse: valid rows; dproj: all rows (the reference is exactly zero on padded rows); dhead_w: one element per row.
    Where d head_w is exactly zero in the reference (one real key per row: its weight is 1 whatever head_w is) no relative error
    exists; the device's value is then measured against sum over the valid rows of |dfeat_i| |feat_i|, the size of the two
    terms (dO . v_j, dO . o_i) whose difference every contribution to it is a multiple of."""
    v = inp["qmask"].bool()
    allr = torch.ones_like(v)
    r = {"feat": _rows(dev["feat"], ref["feat"], v, v), "feat_pad": _rows(dev["feat"], ref["feat"], ~v, v),
         "lse": _rows(dev["lse"], ref["lse"], v, v)}
    if "dproj" in ref:
        r["dproj"] = _rows(dev["dproj"], ref["dproj"], allr, v)
        four = torch.ones(4, dtype=torch.bool)
        if float(ref["dhead_w"].abs().max()) == 0.0:
            size = (inp["dfeat"].double().norm(dim=-1) * ref["feat"].double().norm(dim=-1))[v].sum()
            e = float(dev["dhead_w"].double().abs().max() / size)
            r["dhead_w"] = (e, e)
        else:
            r["dhead_w"] = _rows(dev["dhead_w"].reshape(4, 1), ref["dhead_w"].reshape(4, 1), four, four)
    return r


def run_core(inp, dtype, backward, hooks=None):
    """`core` on the inputs cast to dtype (+ its autograd gradients of sum(feat * dfeat)) -> dict as `metrics` wants it."""
    x = {k: inp[k].to(dtype) for k in ("proj", "rot", "trans", "mask", "head_w", "dfeat")}
    if not backward:
        with torch.no_grad():
            feat, lse = core(x["proj"], x["rot"], x["trans"], x["mask"], x["head_w"], hooks)
        return dict(feat=feat, lse=lse)
    with torch.enable_grad():     # (test modules switch autograd off for the process)
        proj, hw = x["proj"].clone().requires_grad_(True), x["head_w"].clone().requires_grad_(True)
        feat, lse = core(proj, x["rot"], x["trans"], x["mask"], hw, hooks)
        dproj, dhw = torch.autograd.grad((feat * x["dfeat"]).sum(), (proj, hw))
    return dict(feat=feat.detach(), lse=lse.detach(), dproj=dproj, dhead_w=dhw)


def effective_keys(inp):
    """From the fp64 reference: per head, the median over the valid query rows of exp(entropy of the attention weights) /
    (number of real keys of the row's sample)."""
    seen = {}
    x = {k: inp[k].double() for k in ("proj", "rot", "trans", "mask", "head_w")}
    with torch.no_grad():
        core(x["proj"], x["rot"], x["trans"], x["mask"], x["head_w"], {"probs": lambda a, h: seen.__setitem__(h, a)})
    B, L = inp["mask"].shape
    G = inp["proj"].shape[0] // L
    nv = inp["mask"].sum(1)[torch.arange(G) % B].double()[:, None].expand(G, L)
    v = inp["qmask"].bool().view(G, L)
    out = []
    for h in range(4):
        a = seen[h]
        neff = torch.exp(-(a * torch.log(a.clamp_min(1e-300))).sum(-1))
        out.append(float((neff / nv)[v].median()))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, fp64 outputs, {quantity: (gate of max, gate of rel)}, {quantity: floors}) of a case; computed once, shared,
    never modified.  Asserts the condition on the compact inputs: attention spread over at least a quarter of the real keys
    (median over the valid rows, heads 0 - 2) -- without it the mask faults are invisible (chain inputs: attending one padded
    key changes the output by 6e-9)."""
    inp = inputs(case.B, case.ngroups, case.L, case.kind, case.seed)
    if case.kind == "compact":
        spread = effective_keys(inp)
        assert min(spread[:3]) >= 0.25, (case.id, spread)
    bwd = case.bwd is not None
    ref = run_core(inp, torch.float64, bwd)
    floor = metrics(run_core(inp, torch.float32, bwd), ref, inp)
    gate = {k: tuple(max(FACTOR * f, ULPS) for f in v) for k, v in floor.items()}
    return inp, ref, gate, floor


def check(tag, got, gate):
    """Every quantity of `got` (from `metrics`) under its gate, max and rel-L2."""
    bad = {k: (got[k], gate[k]) for k in got if not (got[k][0] <= gate[k][0] and got[k][1] <= gate[k][1])}
    assert not bad, (tag, bad)


def report_line(tag, got, floor):
    x = lambda a, f: f"x{a / f:.1f}" if f > 0 else "-"
    return f"{tag}: " + " | ".join(f"{k} {got[k][0]:.2e}/{got[k][1]:.2e} ({x(got[k][0], floor[k][0])}/{x(got[k][1], floor[k][1])} of floor)"
                                   for k in got)


def slices_used(L, nsplit):
    """(slices that hold keys, slices past L) when ceil(L / 32) tiles are cut into nsplit slices of whole tiles."""
    ntile = (L + 31) // 32
    per = (ntile + nsplit - 1) // nsplit
    used = (ntile + per - 1) // per
    return used, nsplit - used
