"""The key-padding mask of the tiled attention's fixed-anchor loop is supplied by the WRITERS of the fragments: every V^T entry of an
invalid key slot (a token the mask removes, or a slot behind the learned bias key in a sequence's last tile) is zero, the entry of
the denominator row 24 included, and K of the slots behind the bias key is the bias key's (k_gemm.hip epilogue_v_flash,
write_bias_slots); the loop itself masks no score (k_flash.hip).  The robust loop still masks scores.

Every case runs the trunk forward against the CPU oracle at the gate of `tests/test_k_fragments_compact_gpu.py` (rel-L2 < TOL_FWD
on every trace; a second call gives the same bits) with every attention form -- k_flash + out-projection (`flash_proj` 0),
k_flash_proj (`flash_proj` 2, `flash_proj_form` 4), k_flash_proj8 (`flash_proj_form` 8) -- in the fixed-anchor and the robust loop
(`attention_path` 0 / 1) and both tile walk orders, on a workspace filled with 0xFF bytes, and compares the forms with that file's
bounds: q64 == separate kernels bit for bit in natural order, q128 against them < 2e-5, robust against fixed-anchor < 6e-3.

The oracle's own fp32 rounding at these shapes (fp32 against fp64 evaluation, CPU; out and every trace, rel-L2): <= 6.6e-7 at the
temporal tails, <= 7.7e-5 at L = 40 with the masks (the IPA stack of the fully masked samples) -- two orders of magnitude inside
TOL_FWD at the least.
"""
import pytest
import torch

from conftest import rel_l2
from test_gpu_parity import TOL_FWD, _fwd_case, _profiled_forward

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FORMS = (("separate", {"flash_proj": 0}, "flash_T"),
         ("q64", {"flash_proj": 2, "flash_proj_form": 4}, "flash_proj_T@q64"),
         ("q128", {"flash_proj": 2, "flash_proj_form": 8}, "flash_proj_T@q128"))

# L = 40, T = 8, three samples.  Sample 0: the last 8 residues padded (32..39, 33 among them: tile 1, beside the bias key at slot 8)
# and single residues masked inside tile 0 (3, 17); sample 1: residues 0..31 masked and 32..39 VALID -- all of tile 0 masked, nothing
# to anchor to, so its jobs take the robust loop (with 32..39 padded as well the sample would be sample 2 again); sample 2: every
# residue masked -- its sequences see only the learned bias key.  The padding is applied here, per sample (n_pad = 0 in _fwd_case).
L40_MASKED = [(0, l) for l in (3, 17) + tuple(range(32, 40))] + [(1, l) for l in range(32)] + [(2, l) for l in range(40)]


def _case(B, T, L, n_pad, seed, masked=()):
    """_fwd_case with the residues (b, l) of `masked` masked as padded residues are in the dataset (aatype 0, identity frames)."""
    cfg, sd, kw, dkw = _fwd_case(B, T, L, n_pad, seed)
    if masked:
        mask, aat = kw["mask"].clone(), kw["aatype"].clone()
        frames = {k: (kw[k][0].clone(), kw[k][1].clone()) for k in ("start_frames", "end_frames")}
        for b, l in masked:
            mask[b, :, l] = 0
            aat[b, l] = 0
            for R, t in frames.values():
                R[b, l] = torch.eye(3)
                t[b, l] = 0
        kw = dict(kw, mask=mask, aatype=aat, **frames)
        dev = dkw["x"].device
        dkw = {k: (tuple(u.to(dev) for u in v) if isinstance(v, tuple) else v.to(dev)) for k, v in kw.items()}
    return cfg, sd, kw, dkw


def _run_all_forms(case, tag):
    """The forward in every (form, loop, tile order) against the oracle (computed once); {(form, loop, order): output}."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.model import LatentMDGenModel
    cfg, sd, kw, dkw = case
    L = kw["x"].shape[2]
    ref, rtr = O.forward(sd, O.cfg_dict(cfg), return_trace=True, **kw)
    outs = {}
    for form, opts, kernel in FORMS:
        for robust in (0, 1):
            for rotate in ((1, 0) if not robust else (0,)):   # (the robust loop ignores the walk order)
                m = LatentMDGenModel(cfg)
                m.load_state_dict(sd)
                for k, v in dict(opts, attention_path=robust, flash_rotate=rotate).items():
                    m.set_option(k, v)
                out, tr, ran = _profiled_forward(m, dkw)
                key = (form, robust, rotate)
                assert torch.isfinite(out).all(), key
                assert kernel in ran and sum(k.startswith(("flash_T", "flash_proj_T")) for k in ran) == 1, (key, ran)
                if L > 8:   # the residue axis and the IPA stack go through the same writers and readers
                    assert any(k.startswith(("flash_L", "flash_proj_L")) for k in ran) and any(k.startswith("ipa.flash") for k in ran), ran
                rep = {k: rel_l2(tr[k].cpu(), rtr[k]) for k in ["ipa_out"] + [f"h{i}" for i in range(cfg.num_layers + 1)]}
                rep["out"] = rel_l2(out.cpu(), ref)
                print(tag, key, {k: f"{v:.2e}" for k, v in rep.items()})
                for k, v in rep.items():
                    assert v < TOL_FWD, (key, k, v)
                assert torch.equal(m.forward(**dkw), out), key   # a second call on the same context: the same bits
                outs[key] = out.cpu()
                del m
    return outs


def _check_forms_against_each_other(outs):
    for robust in (0, 1):
        nat = {f: outs[(f, robust, 0)] for f, _, _ in FORMS}
        # same operands into the same MFMAs in the same order: the same bits
        assert torch.equal(nat["q64"], nat["separate"]), robust
        e = rel_l2(nat["q128"], nat["separate"])
        print(f"robust {robust}: 128-query form vs separate kernels, natural tile order: {e:.2e}")
        assert e < 2e-5
    for f, _, _ in FORMS:
        e_rot, e_rob = rel_l2(outs[(f, 0, 1)], outs[(f, 0, 0)]), rel_l2(outs[(f, 1, 0)], outs[(f, 0, 0)])
        print(f"{f}: rotated vs natural tile order {e_rot:.2e}, robust vs fixed-anchor loop {e_rob:.2e}")
        assert e_rot < 2e-3 and e_rob < 6e-3


@pytest.mark.parametrize("T", [33, 40, 63, 65, 97])
def test_temporal_tails(T):
    """L = 4, B = 2: the last key tile holds 1, 8, 31, 1, 1 real keys beside the bias key and 30, 23, 0, 30, 30 invalid slots; two,
    three (65: the paired loop's tail tile) and four (97: tile rotation active) tiles."""
    _check_forms_against_each_other(_run_all_forms(_case(2, T, 4, 0, 7300 + T), (2, T, 4)))


def test_residue_axis_masks():
    """L = 40, T = 8, B = 3 (L40_MASKED; 8 padded residues in sample 0): masked keys inside full and partial tiles of the residue
    axis and the IPA stack, a sample whose first tile is fully masked (nothing to anchor to: its jobs take the robust loop), a
    sample that sees only the bias key; the temporal sequences of masked residues consist of masked tokens only."""
    _check_forms_against_each_other(_run_all_forms(_case(3, 8, 40, 0, 7340, L40_MASKED), (3, 8, 40)))


# ---- fragment invariants ------------------------------------------------------------------------------------------------------
# Layout (k_gemm.hip write_bias_slots, restated once): fragment tile ft = (seq * 16 + head) * nt + tile, nt = len / 32 + 1 tiles per
# (sequence, head); the bias key is key slot len % 32 of tile len / 32.
#   K tile, 1536 B: k-step 0 = 64 x 16 B at (hh * 32 + slot) * 16, k-step 1 = 64 x 8 B at 1024 + (hh * 32 + slot) * 8 (hh: feature half).
#   V^T tile, 1600 B: 16-byte rows [k-step ks 2][key half hk 2][row d 25] of 8 bf16; key slot sl is element r & 7 of k-step r >> 3,
#   key half (sl >> 2) & 1, where r = (sl & 3) + 4 (sl >> 3).  Row 24 is the denominator's.
K_TILE, V_TILE, HEADS = 1536, 1600, 16


def _fragments(m, B, T, L):
    """(K [seq, head, tile, slot, 24 bytes], V^T [seq, head, tile, row 25, slot 32] as bf16 bit patterns) of the temporal axis: what
    the last trunk layer's temporal sub-layer left in the workspace (sequence b * L + l, len = T)."""
    lay = m.workspace_layout(B, T, L, 1, B == 1)
    (ws,) = m._ws.values()
    nseq, nt = B * L, T // 32 + 1
    kb = ws[lay.kf:lay.kf + nseq * HEADS * nt * K_TILE].cpu().view(nseq, HEADS, nt, K_TILE)
    k0 = kb[..., :1024].reshape(nseq, HEADS, nt, 2, 32, 16)
    k1 = kb[..., 1024:].reshape(nseq, HEADS, nt, 2, 32, 8)
    K = torch.cat([k0, k1], -1).permute(0, 1, 2, 4, 3, 5).reshape(nseq, HEADS, nt, 32, 48)
    vb = ws[lay.vf:lay.vf + nseq * HEADS * nt * V_TILE].cpu().view(torch.int16).view(nseq, HEADS, nt, 2, 2, 25, 8)
    V = torch.zeros(nseq, HEADS, nt, 25, 32, dtype=torch.int16)
    for sl in range(32):
        r = (sl & 3) + 4 * (sl >> 3)
        V[..., sl] = vb[:, :, :, r >> 3, (sl >> 2) & 1, :, r & 7]
    return K, V


@pytest.mark.parametrize("shape", ["T33", "L40_masked"])
def test_fragment_invariants(shape):
    """After one forward on a 0xFF-filled workspace, per (sequence, head, tile) of the temporal fragments: every V^T entry of an
    invalid slot is 0 in rows 0..24; row 24 is 1.0 exactly at the valid slots; K at the slots behind the bias key equals the bias
    key's.  (The residue-axis fragments of the L = 40 case are overwritten by the temporal sub-layer that follows them: the oracle
    gates above cover them; here the temporal sequences of masked residues hold masked tokens in front of the bias key.)"""
    from mdgen_amd.model import LatentMDGenModel
    B, T, L, n_pad, masked = (2, 33, 4, 0, ()) if shape == "T33" else (3, 8, 40, 0, L40_MASKED)
    cfg, sd, kw, dkw = _case(B, T, L, n_pad, 7400 + T, masked)
    for form, opts, _ in FORMS:
        m = LatentMDGenModel(cfg)
        m.load_state_dict(sd)
        for k, v in dict(opts, streams=1).items():   # one view: the whole batch in one fragment region
            m.set_option(k, v)
        out, _, _ = _profiled_forward(m, dkw)
        assert torch.isfinite(out).all()
        K, V = _fragments(m, B, T, L)
        nt, kt, sl = T // 32 + 1, T // 32, T % 32
        valid = torch.zeros(B * L, nt * 32, dtype=torch.bool)
        valid[:, :T] = kw["mask"].permute(0, 2, 1).reshape(B * L, T) != 0   # sequence b * L + l, position t
        valid[:, T] = True                                                  # the learned bias key
        valid = valid.view(B * L, 1, nt, 1, 32).expand(B * L, HEADS, nt, 25, 32)
        assert (~valid).any() and valid.any()
        assert (V[~valid] == 0).all(), form
        ones = V[:, :, :, 24, :]
        assert (ones[valid[:, :, :, 24, :]] == 0x3f80).all() and (ones[~valid[:, :, :, 24, :]] == 0).all(), form
        assert sl < 31
        assert torch.equal(K[:, :, kt, sl + 1:], K[:, :, kt, sl:sl + 1].expand_as(K[:, :, kt, sl + 1:])), form
        del m
