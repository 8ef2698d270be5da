"""The compact K attention fragments (1536 B per 32-key tile: k-step 0, then the four real bf16 of k-step 1; the constant half of
k-step 1 lives in registers of the attention kernels) at the sizes where a writer or a reader of the layout takes another path.

Every case runs the trunk forward against the CPU oracle at the gate `test_flash_proj_kernel_vs_separate_kernels_and_oracle` uses
(rel-L2 < TOL_FWD on every trace), with every attention form the options select -- k_flash + out-projection (`flash_proj` 0),
k_flash_proj (`flash_proj` 2, `flash_proj_form` 4) and k_flash_proj8 (`flash_proj_form` 8); all three can be forced at these
sizes -- in the fixed-anchor and the robust loop (`attention_path` 0 / 1), on a workspace filled with 0xFF bytes.  Forms that sum
every query's keys in the same order on the same operands are compared for exact equality: k_flash + projection and k_flash_proj
in natural tile order (both loops: the robust loop always walks in natural order); the 128-query form against them to fp32
rounding (2e-5), the robust loop against the fixed-anchor loop to 6e-3 (P rounded to bf16 around another shift) -- the bounds of
the test named above.
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


def _run_all_forms(B, T, L, n_pad, seed):
    """The forward in every (form, loop, tile order) against the oracle (computed once); {(form, loop, order): output}."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.model import LatentMDGenModel
    cfg, sd, kw, dkw = _fwd_case(B, T, L, n_pad, seed)
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
                print((B, T, L, n_pad), key, {k: f"{v:.2e}" for k, v in rep.items()})
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


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [31, 32, 64, 33, 65, 160])
def test_temporal_tile_shapes(T, B):
    """L = 4 (the residue axis runs k_ln_qkv_attn4: only the temporal axis is tiled).  T 31: keys + bias key fill exactly one tile;
    32, 64: the bias key alone in the last tile (the rank-1 path reading its K slot, kb0 / kb1; at 64 the tile is one no panel
    epilogue touched, zeroed by the bias-slot writer); 33, 65: a last tile of one key and the bias key, even and odd tile counts
    through the paired loop and its tail tile; 160: six tiles, tile rotation active."""
    _check_forms_against_each_other(_run_all_forms(B, T, 4, 0, 900 + T))


def test_residue_axis_with_padded_residues():
    """L = 40 with 8 padded residues, T = 8: key-padding words in the residue axis' last tile (and the IPA stack's), and a padded
    residue's temporal sequence has no valid key but the bias key (the direct bias_v path; the robust loop with it forced)."""
    outs = _run_all_forms(1, 8, 40, 8, 940)
    _check_forms_against_each_other(outs)
