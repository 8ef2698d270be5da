"""Per-layer, per-row parity of the sampler's forward against the fp64 oracle (an ordinary module the GPU tests import).

The whole-tensor gates of tests/test_gpu_parity.py compare the accumulated residual stream h0 .. h5 with the fp32 oracle.  The
embedding + IPA error (~4.5e-3) dominates those traces and every trunk layer adds ~1e-5 on top of it, so a trunk kernel that is
wrong in a few rows, or in one tile, stays under the 1e-2 gate.  Here every stage is fed the DEVICE's own input and only what the
stage adds is compared, row by row, with the oracle's fp64 evaluation of that stage:

  ipa      ipa_out                        vs  run_ipa (the whole IPA stack: the library has no per-layer IPA trace)
  embed    h0 - ipa_out                   vs  embed(x, x_cond, x_cond_mask)
  layer i  h_{i+1} - h_i                  vs  trunk_layer(h_i) - h_i        (h_i the device's)
  final    out                            vs  final_layer(h_nl)             (h_nl the device's)
  euler    x2 - x0 of two Euler steps     vs  the oracle's two steps in fp64 (calls without a trace)

Per row (b, t, l): e = |d_dev - d_ref| / rms_rows |d_ref|.  A stage reports the max and the rms of e, the row of the max, and
the worst group mean for three groupings: per sample, per (sample, 64-row block of the temporal axis) and per (sample, 32-row
block of the residue axis) -- the tiles of the attention kernels, so a wrong tile shows up as a group.  Trunk rows are all gated,
padded query rows included (the whole-tensor tests include them too); IPA rows of padded residues are not defined by the
reference (test_ipa_table_of_all_steps_vs_oracle) and only have to be finite.
"""
import torch

from oracle import mdgen_oracle as O

# Gates on (max e, worst group mean) per stage, set on the MI355X from every forward test and sweep case (43 traced calls, 182
# trunk layers, 8 two-step rollouts).  Worst measured (max / group mean): ipa 1.10e-2 / 5.3e-3, embed 2.4e-7 / 2.0e-7 (fp32
# arithmetic), trunk 4.75e-3 / 4.0e-3, final 4.3e-3 / 2.6e-3, euler 8.1e-3 / 5.7e-3.  Every trunk form measured 3.5e-3 .. 4.75e-3,
# so the trunk has one class.  Gates sit at about twice the worst, except the trunk's max: at 1.6x it stays 10x below the smallest
# response to the faults of tests/test_layer_parity_cpu.py (0.080), which also checks that the clean bf16 stand-in passes them.
GATES = {
    "ipa": (2.2e-2, 1.1e-2),
    "embed": (5e-7, 4e-7),
    "trunk": (7.5e-3, 7.5e-3),
    "final": (9e-3, 5e-3),
    "euler": (1.6e-2, 1.2e-2),
}
# trunk layers checked at shapes above this many rows: the first and the last (all layers of a call run the same kernel forms)
ALL_LAYERS_MAX_ROWS = 16384


def _group_means(e, valid, axis, size):
    """Worst mean of e over (sample, block of `size` rows along `axis`) groups -> (value, (b, start)); axis None: per sample."""
    worst, at = -1.0, None
    n = 1 if axis is None else e.shape[axis]
    step = n if axis is None else size
    for s in range(0, n, step):
        sl = [slice(None)] * e.dim()
        if axis is not None:
            sl[axis] = slice(s, s + size)
        eb, vb = e[tuple(sl)], valid[tuple(sl)]
        for b in range(e.shape[0]):
            k = int(vb[b].sum())
            if k == 0:
                continue
            m = float(eb[b][vb[b]].sum()) / k
            if m > worst:
                worst, at = m, (b, s)
    return worst, at


def stage_errors(d_dev, d_ref, valid=None):
    """Row metric and its summary.  d_dev, d_ref [B, T, L, C] (or [B, L, C]: no temporal axis); valid: rows to gate (bool, the
    row shape; None: all)."""
    d_dev, d_ref = d_dev.double(), d_ref.double()
    rows = d_ref.shape[:-1]
    valid = torch.ones(rows, dtype=torch.bool) if valid is None else valid.expand(rows)
    scale = float(d_ref.norm(dim=-1)[valid].pow(2).mean().sqrt().clamp_min(1e-30))
    e = (d_dev - d_ref).norm(dim=-1) / scale
    e = torch.where(valid, e, torch.zeros(()).double())
    ev = e[valid]
    i = int(torch.argmax(e))
    loc = list(torch.unravel_index(torch.tensor(i), rows))
    loc = tuple(int(v) for v in (loc if len(rows) == 3 else [loc[0], -1, loc[1]]))
    r = {"max": float(ev.max()), "rms": float(ev.pow(2).mean().sqrt()), "at": loc, "finite": bool(torch.isfinite(d_dev).all())}
    t_axis, l_axis = (1, 2) if len(rows) == 3 else (None, 1)
    groups = {"sample": _group_means(e, valid, None, 0), "l32": _group_means(e, valid, l_axis, 32)}
    if t_axis is not None:
        groups["t64"] = _group_means(e, valid, t_axis, 64)
    r["group"] = max(groups.items(), key=lambda kv: kv[1][0])   # (grouping, (mean, (b, start)))
    return r


def _fmt(name, r):
    g, (m, at) = r["group"]
    return f"{name} {r['max']:.2e}/{r['rms']:.2e}@{r['at']} {g}{at}={m:.2e}"


def report_line(tag, rep):
    return f"{tag} per-row max/rms@(b,t,l), worst group mean: " + " | ".join(_fmt(k, r) for k, r in rep.items())


def gate_class(stage):
    return "trunk" if stage.startswith("layer") else stage


def check(tag, rep, gates=None):
    """Print the report line and assert every stage's max and worst group mean under its class's gate."""
    gates = gates or GATES
    print(report_line(tag, rep))
    for k, r in rep.items():
        gmax, ggrp = gates[gate_class(k)]
        assert r["finite"], (tag, k, "non-finite rows")
        assert r["max"] < gmax and r["group"][1][0] < ggrp, (tag, k, _fmt(k, r), (gmax, ggrp))


def trunk_layers(nl, rows, layers=None):
    if layers is not None:
        return list(layers)
    return list(range(nl)) if rows <= ALL_LAYERS_MAX_ROWS else [0, nl - 1]


def forward_stages(cfg, sd, kw, out, trace, cd=None, layers=None):
    """{stage: summary} of one traced forward.  cfg: ModelConfig; sd: the state dict; kw: the oracle's (host) inputs; out, trace:
    the device's velocity and trace (ipa_out, h0 .. h_nl); cd: the oracle's cfg dict (default O.cfg_dict(cfg)); layers: trunk
    layers to check (default: all at small shapes, the first and the last above ALL_LAYERS_MAX_ROWS rows)."""
    cd = dict(cd if cd is not None else O.cfg_dict(cfg))
    P, (x, t, mask, sf, ef, xc) = O.to_fp64(sd, kw["x"], kw["t"], kw["mask"], kw["start_frames"], kw["end_frames"], kw["x_cond"])
    if torch.is_tensor(cd.get("quat_sign")):
        cd["quat_sign"] = cd["quat_sign"].double()
    tr = {k: v.detach().cpu().double() for k, v in trace.items()}
    nl, H = cd["num_layers"], cd["mha_heads"]
    B, T, L = x.shape[:3]
    te = O.temb(P, cd, t)
    rep = {}
    ipa_ref = O.run_ipa(P, cd, te[:, 0], mask[:, 0], sf, ef, kw["aatype"])
    valid = kw["mask"][:, 0].bool()
    rep["ipa"] = stage_errors(tr["ipa_out"], ipa_ref, valid)
    rep["ipa"]["finite"] = bool(torch.isfinite(tr["ipa_out"]).all())       # padded rows: finite, not gated
    del ipa_ref
    rep["embed"] = stage_errors(tr["h0"] - tr["ipa_out"][:, None], O.embed(P, cd, x, xc, kw["x_cond_mask"]))
    for i in trunk_layers(nl, B * T * L, layers):
        h = tr[f"h{i}"]
        rep[f"layer{i}"] = stage_errors(tr[f"h{i + 1}"] - h, O.trunk_layer(P, f"layers.{i}.", h, te, mask, H) - h)
    rep["final"] = stage_errors(out.detach().cpu(), O.final_layer(P, tr[f"h{nl}"], te))
    return rep


def check_forward(tag, cfg, sd, kw, out, trace, cd=None, layers=None, gates=None):
    rep = forward_stages(cfg, sd, kw, out, trace, cd=cd, layers=layers)
    check(tag, rep, gates)
    return rep


def check_euler(tag, dx_dev, dx_ref, gates=None):
    """x2 - x0 of a two-step rollout against the oracle's two steps in fp64 (`dx_ref`), per row."""
    rep = {"euler": stage_errors(dx_dev.detach().cpu(), dx_ref)}
    check(tag, rep, gates)
    return rep
