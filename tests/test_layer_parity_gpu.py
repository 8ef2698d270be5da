"""Edge sweep of the trunk's kernel forms, gated per layer and per row against the fp64 oracle (tests/layer_parity.py).

Each case sits at a tile edge of the form it was chosen for (read from api.hip's dispatch and the kernels: 64-query chunks,
128-query chunks of k_flash_proj8 at len >= 512, 32-key tiles that also hold the learned bias key, 32-row panels, the L = 4 and
L <= 8 residue paths), has B > 1 samples with their own t and their own number of padded residues -- one of them, where the
case says so, with a residue-axis key tile that is all padding -- and asserts through `mdgen_debug_dispatch_plan` that the call
runs the form it was chosen for, so that a threshold change cannot move the sweep off its target silently.  The workspace is
filled with 0xFF bytes first (NaN in bf16 and fp32): whatever the kernels read must have been written by the call.
"""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import layer_parity as LP  # noqa: E402

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# (name, B, T, L, padded residues per sample, kernel classes the plan must contain)
CASES = [
    # temporal k_flash_proj (64 queries): T = 64 + 1, a one-query tail chunk; 66 keys = 3 key tiles.  Residue axis L 128: 129 keys, 5 tiles,
    # sample 1's last 33 residues padded -> its key tile 96..127 is all padding
    ("q64T_T65_L128", 2, 65, 128, (0, 33), ("flash_proj_T@q64", "flash_L", "mlp@p4")),
    # temporal k_flash_proj8 (128 queries, len >= 512): T 512, the bias key opens key tile 17; residue axis k_flash_proj at L 32 (bias opens tile 2)
    ("q128T_T512_L32", 2, 512, 32, (0, 3), ("flash_proj_T@q128", "flash_proj_L@q64", "mlp")),
    # L = 4: k_ln_qkv_attn4 in its 32-row form; T 65; sample 2 has one real residue
    ("attn4_h32_T65_L4", 3, 65, 4, (0, 1, 3), ("attn_L_fused@h32", "ln_qkv_T@h32x2")),
    # micro residue attention (L <= 8) at L 8 and L 5
    ("micro_T64_L8", 2, 64, 8, (0, 1), ("ln_qkv_L", "proj_L")),
    ("micro_T33_L5", 3, 33, 5, (0, 2, 4), ("ln_qkv_L", "proj_L")),
    # residue-axis k_flash_proj (64 queries): L 65, a one-query tail chunk, 66 keys = 3 tiles; sample 2's residues 32..64 padded -> tile 32..63
    # is all padding; four-wave panel MLP
    ("q64L_T100_L65", 3, 100, 65, (0, 1, 33), ("flash_proj_L@q64", "proj_mlp@p4")),
    # tiled residue axis, separate k_flash: L 33 (34 keys: tile 2 holds one residue and the bias key), split q, k | v panels
    ("tiledL_T40_L33", 2, 40, 33, (0, 1), ("flash_L", "ln_qkv_L@p8x2")),
    # L 32 (bias key alone in tile 2), T 97 (a 33-query tail chunk), eight-wave panel forms; sample 1 has one real residue
    ("tiledL_T97_L32", 2, 97, 32, (0, 31), ("flash_L", "ln_qkv_L@p8", "proj_mlp@p8")),
    # 32-row panels of the residue-axis q, k | v launch, L 9
    ("h32_T64_L9", 2, 64, 9, (0, 8), ("ln_qkv_L@h32x2", "flash_L")),
]


def _inputs(cfg, B, T, L, pads, seed):
    """synth_forward_inputs with its own number of padded residues per sample (dataset.py:80-89: mask 0, aatype 0, identity frames)."""
    from mdgen_amd.synthetic import synth_forward_inputs
    inp = synth_forward_inputs(cfg, B, T, L, 0, seed)
    mask = torch.ones(B, L)
    for b, n in enumerate(pads):
        if n:
            mask[b, L - n:] = 0
            inp["aatype"][b, L - n:] = 0
            for k in ("start_rot", "end_rot"):
                inp[k][b, L - n:] = torch.eye(3)
            for k in ("start_trans", "end_trans"):
                inp[k][b, L - n:] = 0
    inp["mask"] = mask[:, None].expand(B, T, L).contiguous()
    return dict(x=inp["x"], t=inp["t"], mask=inp["mask"], start_frames=(inp["start_rot"], inp["start_trans"]),
                end_frames=(inp["end_rot"], inp["end_trans"]), x_cond=inp["x_cond"], x_cond_mask=inp["x_cond_mask"],
                aatype=inp["aatype"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_trunk_forms_at_tile_edges_per_layer_vs_fp64(case):
    from mdgen_amd._lib import dispatch_plan
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.model import LatentMDGenModel
    from mdgen_amd.synthetic import synth_state_dict
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    dev = torch.device("cuda")
    name, B, T, L, pads, forms = case
    assert len(pads) == B and len(set(pads)) > 1
    cfg = ModelConfig.forward_sim(num_frames=T, crop=max(L, 4))
    sd = synth_state_dict(cfg, 5)
    kw = _inputs(cfg, B, T, L, pads, 7000 + 7 * T + L)
    assert len(set(kw["t"].tolist())) == B                     # per-sample t
    dkw = {k: (tuple(u.to(dev) for u in v) if isinstance(v, tuple) else v.to(dev)) for k, v in kw.items()}
    m = LatentMDGenModel(cfg)
    m.load_state_dict(sd)
    m.forward(**dkw)                                           # allocates (and caches) the workspace of this shape
    for ws in m._ws.values():
        ws.view(torch.uint8).fill_(0xFF)
    m.profile(True)
    try:
        out, tr = m.forward(**dkw, return_trace=True)
        torch.cuda.synchronize()
        ran = {k: v["count"] for k, v in m.profile_report().items()}
        info = m.context_info
    finally:
        m.profile(False)
    want = dispatch_plan(B, T, L, mode=3, ncu=info["ncu"], xcd_round_robin=bool(info["xcd_round_robin"]))
    planned = dict(want["prepare"])
    for vw in want["views"]:
        for k, n in vw["classes"].items():
            planned[k] = planned.get(k, 0) + n
    assert ran == planned, (name, ran, planned)
    for f in forms:
        assert planned.get(f) == cfg.num_layers, (name, f, planned)
    assert torch.isfinite(out).all()
    LP.check_forward(f"{name} pads {pads}", cfg, sd, kw, out, tr)
