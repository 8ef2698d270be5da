"""CPU: pin the oracle (oracle/mdgen_oracle.py) against golden vectors produced by the reference
itself (oracle/gen_golden.py).  fp32 tolerances: the reference's own thread-order noise is
rel-L2 3.3e-7."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, weights_for, rel_l2
from oracle import mdgen_oracle as O

torch.set_grad_enabled(False)


def _torsions_close(got, ref, mask, atol):
    """Torsions (sin, cos) [..., L, 7, 2]: every entry compared, masked or not, except one.  The pre-omega angle of residue 0
    (torsion 0) is built from the zero padding before the chain: a degenerate frame, whose value is the host's last-bit rounding
    amplified to O(1) (the CPU math library's vector square root is not correctly rounded, and its last bit follows the host's
    code path).  That entry must be masked and finite; its value is not compared."""
    keep = torch.ones(got.shape[:-1], dtype=torch.bool)
    keep[..., 0, 0] = False
    return (bool((torch.broadcast_to(mask, got.shape[:-1])[..., 0, 0] == 0).all()) and bool(torch.isfinite(got).all())
            and torch.allclose(got[keep], ref[keep], atol=atol))


def _fwd_kwargs(g):
    return dict(
        x=g["x"], t=g["t"], mask=g["mask"],
        start_frames=(g["start_rot"], g["start_trans"]), end_frames=(g["end_rot"], g["end_trans"]),
        x_cond=g["x_cond"], x_cond_mask=g["x_cond_mask"], aatype=g["aatype"])


@pytest.mark.parametrize("name", ["fwd_tiny_sim", "fwd_tiny_tps", "fwd_full_sim", "fwd_full_pep",
                                  "fwd_full_atlas", "fwd_full_tps"])
def test_forward_matches_reference(name):
    g = load_golden(name)
    cfg, sd = weights_for(g)
    cd = O.cfg_dict(cfg)
    if cfg.tps_condition:   # the relative frames' quaternion signs as the reference drew them (LAPACK's, host-dependent)
        cd["quat_sign"] = g["rel7"]
    out, tr = O.forward(sd, cd, return_trace=True, **_fwd_kwargs(g))
    for k in ("ipa_out", "h0", "h1", f"h{cfg.num_layers}"):
        if k in g:
            assert rel_l2(tr[k], g[k]) < 2e-5, k
    assert rel_l2(out, g["out"]) < 2e-5
    assert (out - g["out"]).abs().max() < 1e-4 * g["out"].pow(2).mean().sqrt() * 10


def test_padded_sequences_are_finite():
    g = load_golden("fwd_full_sim")
    assert torch.isfinite(g["out"]).all()
    assert (g["mask"] == 0).any()


def test_rigid_ops():
    g = load_golden("rigid_ops")
    R, t = O.rigid_compose(g["R1"], g["t1"], g["R2"], g["t2"])
    assert torch.allclose(R, g["comp_R"], atol=1e-6) and torch.allclose(t, g["comp_t"], atol=1e-5)
    R, t = O.rigid_invert(g["R1"], g["t1"])
    assert torch.allclose(R, g["inv_R"], atol=1e-6) and torch.allclose(t, g["inv_t"], atol=1e-5)
    assert torch.allclose(O.rigid_apply(g["R1"], g["t1"], g["p"]), g["apply"], atol=1e-5)
    assert torch.allclose(O.rigid_invert_apply(g["R1"], g["t1"], g["p"]), g["invert_apply"], atol=1e-5)
    t7 = O.to_tensor_7(g["R1"], g["t1"])
    sgn = torch.sign((t7[:, :4] * g["tensor7"][:, :4]).sum(-1, keepdim=True))   # eigh sign is arbitrary
    assert torch.allclose(t7[:, :4] * sgn, g["tensor7"][:, :4], atol=1e-5)
    assert torch.allclose(t7[:, 4:], g["tensor7"][:, 4:])
    R, t = O.from_tensor_7(g["q7"])
    assert torch.allclose(R, g["from7_R"], atol=1e-6) and torch.allclose(t, g["from7_t"])
    off = O.get_offsets((g["R1"][None, :1, None], g["t1"][None, :1, None]), (g["R2"][None, :, None], g["t2"][None, :, None]))
    sgn = torch.sign((off[..., :4] * g["offsets"][..., :4]).sum(-1, keepdim=True))
    assert torch.allclose(off[..., :4] * sgn, g["offsets"][..., :4], atol=1e-5)
    assert torch.allclose(off[..., 4:], g["offsets"][..., 4:], atol=1e-5)
    R, t = O.from_3_points(g["p3a"], g["p3b"], g["p3c"])
    assert torch.allclose(R, g["f3_R"], atol=1e-6) and torch.allclose(t, g["f3_t"])
    # identities: compose with inverse = identity; quat round trip
    iR, it = O.rigid_invert(g["R1"], g["t1"])
    cR, ct = O.rigid_compose(g["R1"], g["t1"], iR, it)
    assert torch.allclose(cR, torch.eye(3).expand_as(cR), atol=1e-5) and ct.abs().max() < 1e-4
    assert torch.allclose(O.quat_to_rot(O.rot_to_quat(g["R1"])), g["R1"], atol=1e-5)


def test_geometry():
    g = load_golden("geometry")
    B, T, L = g["atom14"].shape[:3]
    aat = g["seqres"][:, None].expand(B, T, L)
    R, t = O.atom14_to_frames(g["atom14"])
    assert torch.allclose(R, g["frames_R"], atol=1e-5) and torch.allclose(t, g["frames_t"])
    a37 = O.atom14_to_atom37(g["atom14"], aat)
    assert torch.allclose(a37, g["atom37"])
    tors, tm = O.atom37_to_torsions(a37, aat)
    assert torch.equal(tm, g["torsion_mask"]) and _torsions_close(tors, g["torsions"], tm, atol=1e-5)
    back = O.frames_torsions_to_atom14(R, t, tors, aat)
    assert torch.allclose(back, g["atom14_back"], atol=1e-4)
    # property: atom14_to_frames(frames_torsions_to_atom14(F, tau)) == F
    R2, t2 = O.atom14_to_frames(back)
    assert torch.allclose(R2, R, atol=1e-4) and torch.allclose(t2, t, atol=1e-4)


@pytest.mark.parametrize("name", ["prep_sim", "prep_tps", "prep_sim_interval"])
def test_prep_batch(name):
    g = load_golden(name)
    batch = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    prep = O.prep_batch(batch, dict(g["cfg"], cond_interval=int(g["cond_interval"])))
    if name == "prep_sim_interval":   # --cond_interval 3 on 8 frames: frames 0, 3, 6 are given (wrapper.py:343-344)
        assert g["x_cond_mask"][0, :, 0].tolist() == [1, 0, 0, 1, 0, 0, 1, 0]
    assert torch.allclose(prep["latents"], g["latents"], atol=2e-5)
    assert torch.allclose(prep["model_kwargs"]["x_cond"], g["x_cond"], atol=2e-5)
    assert torch.equal(prep["model_kwargs"]["x_cond_mask"], g["x_cond_mask"])
    assert torch.equal(prep["loss_mask"].float(), g["loss_mask"].float())
    assert torch.equal(prep["model_kwargs"]["mask"], g["mask"])
    assert torch.allclose(prep["model_kwargs"]["start_frames"][0], g["start_rot"])
    assert torch.allclose(prep["model_kwargs"]["end_frames"][1], g["end_trans"])
    # the real part of every offset quaternion is >= 0 (wrapper.py:309)
    assert (g["latents"][..., 0] >= 0).all()
    # get_batch restatement reproduces the reference's batch from the raw atom14 array
    for b in range(g["atom14"].shape[0]):
        mine = O.get_batch_from_atom14(g["atom14"][b], g["in_seqres"][b])
        assert torch.allclose(mine["rots"], g["in_rots"][b], atol=1e-5)
        assert torch.allclose(mine["torsion_mask"], g["in_torsion_mask"][b])
        assert _torsions_close(mine["torsions"], g["in_torsions"][b], g["in_torsion_mask"][b], atol=1e-5)


@pytest.mark.parametrize("name", ["inference_sim", "inference_tiny"])
def test_inference_and_rollout(name):
    g = load_golden(name)
    cfg, sd = weights_for(g)
    cd = O.cfg_dict(cfg)
    batch0 = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    T = g[f"S{int(g['steps'][0])}_b0_zs"].shape[1]
    for S in [int(s) for s in g["steps"]]:
        cur = dict(batch0)
        blk = 0
        while f"S{S}_b{blk}_zs" in g:
            ex = dict(cur)
            ex["torsions"] = cur["torsions"].expand(-1, T, -1, -1, -1)
            ex["trans"] = cur["trans"].expand(-1, T, -1, -1)
            ex["rots"] = cur["rots"].expand(-1, T, -1, -1, -1)
            atom14, aa, samples = O.inference(sd, cd, ex, g[f"S{S}_b{blk}_zs"], S)
            assert rel_l2(samples, g[f"S{S}_b{blk}_samples"]) < 5e-5, (S, blk)
            assert (atom14 - g[f"S{S}_b{blk}_atom14"]).abs().max() < 2e-3, (S, blk)     # Angstrom
            nxt = O.rollout_glue(g[f"S{S}_b{blk}_atom14"][:, -1], batch0["seqres"])
            assert torch.allclose(nxt["trans"], g[f"S{S}_b{blk}_next_trans"], atol=1e-5)
            assert torch.allclose(nxt["rots"], g[f"S{S}_b{blk}_next_rots"], atol=1e-5)
            assert _torsions_close(nxt["torsions"], g[f"S{S}_b{blk}_next_torsions"], batch0["torsion_mask"][:, None], atol=2e-4)
            cur = dict(cur, trans=g[f"S{S}_b{blk}_next_trans"], rots=g[f"S{S}_b{blk}_next_rots"],
                       torsions=g[f"S{S}_b{blk}_next_torsions"])
            blk += 1


def test_rope_matches_hf_port():
    """The fair-esm rotary embedding is not vendored by the reference ("parity unpinned"); cross-check
    the rotate-half convention of the restatement against the independent HF transformers ESM port."""
    try:
        from transformers.models.esm.modeling_esm import apply_rotary_pos_emb, rotate_half
    except Exception:
        pytest.skip("transformers ESM port not importable")
    torch.manual_seed(0)
    q, k = torch.randn(3, 2, 8, 24), torch.randn(3, 2, 8, 24)
    cos, sin = O.rope_tables(8, 24)
    assert torch.equal(rotate_half(q), O.rotate_half(q))
    hq, hk = apply_rotary_pos_emb(q, k, cos[None], sin[None], unsqueeze_dim=1)
    assert torch.allclose(hq, q * cos + O.rotate_half(q) * sin, atol=1e-6)
    assert torch.allclose(hk, k * cos + O.rotate_half(k) * sin, atol=1e-6)
    # angle table: theta[pos, i] = pos * 10000^(-2 (i mod 12) / 24)
    ang = torch.arange(8)[:, None] * (10000.0 ** (-2 * (torch.arange(24) % 12) / 24.0))[None]
    assert torch.allclose(cos, ang.cos(), atol=1e-6) and torch.allclose(sin, ang.sin(), atol=1e-6)


def test_euler_grid():
    """integrators.py:88 linspace(t0,t1,num_steps) -> S = num_steps-1 Euler steps; dt sums to 1."""
    tg = torch.linspace(0, 1, 50)
    assert len(tg) - 1 == 49 and abs(float((tg[1:] - tg[:-1]).sum()) - 1) < 1e-6


def test_quat_sign_option_is_only_a_sign():
    """to_tensor_7(quat_sign="w_nonneg") (the convention the HIP kernel uses) differs from the eigh-signed
    reference restatement by per-quaternion sign only, i.e. it encodes the same rotations."""
    g = torch.Generator().manual_seed(3)
    q = torch.randn(64, 4, generator=g)
    R = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
    t = torch.randn(64, 3, generator=g)
    a = O.to_tensor_7(R, t)
    b = O.to_tensor_7(R, t, quat_sign="w_nonneg")
    assert (b[:, 0] >= 0).all()
    s = torch.sign((a[:, :4] * b[:, :4]).sum(-1, keepdim=True))
    assert torch.allclose(a[:, :4] * s, b[:, :4], atol=1e-6)
    assert torch.equal(a[:, 4:], b[:, 4:])
    assert torch.allclose(O.quat_to_rot(b[:, :4]), R, atol=1e-5)


@pytest.mark.parametrize("name", ["train_tiny_sim", "train_full_sim"])
def test_training_losses_vs_reference(name):
    """Flow-matching target + masked loss: the oracle's restatement of
    `Transport.training_losses` (transport.py:138-189, path.py:113-135, 177-187) vs the reference's own run with
    the same draws of x0 and t (oracle/gen_golden_train.py)."""
    g = load_golden(name)
    cfg, sd = weights_for(g)
    kw = dict(mask=g["mask"], start_frames=(g["start_rot"], g["start_trans"]), end_frames=(g["start_rot"], g["start_trans"]),
              x_cond=g["x_cond"], x_cond_mask=g["x_cond_mask"], aatype=g["aatype"])
    out = O.training_losses(sd, O.cfg_dict(cfg), g["x1"], g["loss_mask"], kw, g["t"], g["x0"])
    assert rel_l2(out["pred"], g["pred"]) < 2e-5
    assert torch.allclose(out["loss"], g["loss"], rtol=2e-5)
    # the plan itself: endpoints and derivative identities of the GVP path
    xt0, ut0 = O.path_plan(torch.zeros(2), g["x0"], g["x1"])
    xt1, _ = O.path_plan(torch.ones(2), g["x0"], g["x1"])
    assert torch.allclose(xt0, g["x0"], atol=1e-6) and torch.allclose(xt1, g["x1"], atol=1e-6)
    assert torch.allclose(ut0, (math.pi / 2) * g["x1"], atol=1e-5)


@pytest.mark.parametrize("name,shape", [("fwd_cfg4_atlas_full", (1, 250, 256, 16)), ("fwd_cfg2_T1000", (2, 1000, 4, 0)),
                                        ("fwd_cfg1_T100", (1, 100, 4, 0))])
def test_forward_full_size_matches_reference(name, shape):
    """BASELINE.json configs at their FULL per-sample size -- configs[3] (ATLAS crop 256 x 250 frames, B 1, 16 padded
    residues), configs[1]'s regime (tetrapeptide, 1000 frames = 1001 temporal keys, B 2 with distinct t) and configs[0]'s
    shape (B 1, 100 frames): the oracle vs the reference's own run (seeded inputs regenerated here, checked by checksum;
    reference outputs stored sub-sampled)."""
    from mdgen_amd.synthetic import synth_forward_inputs, tensor_checksum
    g = load_golden(name)
    cfg, sd = weights_for(g)
    B, T, L, n_pad = (int(v) for v in g["shape"])
    assert (B, T, L, n_pad) == shape
    inp = synth_forward_inputs(cfg, B, T, L, n_pad, int(g["data_seed"]))
    np.testing.assert_allclose(tensor_checksum(inp), g["input_checksum"].numpy(), rtol=1e-12)
    out, tr = O.forward(sd, O.cfg_dict(cfg), return_trace=True, x=inp["x"], t=inp["t"], mask=inp["mask"],
                        start_frames=(inp["start_rot"], inp["start_trans"]), end_frames=(inp["end_rot"], inp["end_trans"]),
                        x_cond=inp["x_cond"], x_cond_mask=inp["x_cond_mask"], aatype=inp["aatype"])
    st, sl = (int(v) for v in g["sub"])
    ht, hl = (int(v) for v in g["sub_h"])
    nl = cfg.num_layers
    assert rel_l2(out[:, ::st, ::sl], g["out"]) < 2e-5
    assert rel_l2(tr["ipa_out"][:, ::sl], g["ipa_out"]) < 2e-5
    assert rel_l2(tr["h0"][:, ::ht, ::hl], g["h0"]) < 2e-5
    assert rel_l2(tr[f"h{nl}"][:, ::ht, ::hl], g[f"h{nl}"]) < 2e-5
    norms = [float(out.double().norm()), float(tr["ipa_out"].double().norm()), float(tr["h0"].double().norm()),
             float(tr[f"h{nl}"].double().norm())]
    np.testing.assert_allclose(norms, g["norms"].numpy(), rtol=1e-5)


def test_inference_cfg1_shape_matches_reference():
    """BASELINE.json configs[0] (single tetrapeptide, 100 frames, 10 Euler steps, the reference's CPU-runnable case):
    the oracle's inference() vs the reference's own run at that exact shape."""
    g = load_golden("inference_cfg1")
    cfg, sd = weights_for(g)
    B, T, L = (int(v) for v in g["shape"])
    assert (B, T, L, int(g["S"])) == (1, 100, 4, 10)
    batch0 = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    ex = dict(batch0)
    ex["torsions"] = batch0["torsions"].expand(-1, T, -1, -1, -1)
    ex["trans"] = batch0["trans"].expand(-1, T, -1, -1)
    ex["rots"] = batch0["rots"].expand(-1, T, -1, -1, -1)
    zs = torch.randn(B, T, L, cfg.latent_dim, generator=torch.Generator().manual_seed(137))
    a14, _, _ = O.inference(sd, O.cfg_dict(cfg), ex, zs, int(g["S"]))
    d = (a14[:, ::int(g["sub_t"])] - g["atom14"]).abs()
    assert float(d.max()) < 1e-3, float(d.max())


@pytest.mark.parametrize("name,nparams", [("train_grads_sim", 124), ("train_grads_tps", 128)])
def test_training_gradients_vs_reference_autograd(name, nparams):
    """The oracle's autograd (what the GPU gradient tests compare against) pinned to the REFERENCE's own backward pass:
    `training_losses(...)["loss"].mean().backward()` on the full-width 2-layer model (tests/golden/train_grads_{sim,tps}.npz,
    oracle/gen_golden_train.py): every parameter's gradient norm and a strided sample of its entries.  The two-sided (TPS)
    fixture has distinct end frames and four more tensors (latent_to_emb_f / _r); the oracle runs it with the reference's
    own quaternion signs (stored in tests/golden/host_rounding.npz: LAPACK's sign follows the host's BLAS code path)."""
    g = load_golden(name)
    cfg, sd = weights_for(g)
    names = [str(n) for n in g["grad_names"]]
    P = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    end = (g["end_rot"], g["end_trans"]) if "end_rot" in g else (g["start_rot"], g["start_trans"])
    kw = dict(mask=g["mask"], start_frames=(g["start_rot"], g["start_trans"]), end_frames=end,
              x_cond=g["x_cond"], x_cond_mask=g["x_cond_mask"], aatype=g["aatype"])
    cd = O.cfg_dict(cfg)
    if cfg.tps_condition:
        cd["quat_sign"] = load_golden("host_rounding")["train_grads_tps_rel7"]
    with torch.enable_grad():
        out = O.training_losses(P, cd, g["x1"], g["loss_mask"], kw, g["t"], g["x0"])
        out["loss"].mean().backward()
    assert torch.allclose(out["loss"].detach(), g["loss"], rtol=2e-5)
    assert len(names) == nparams and "pos_embed" not in names        # frozen buffer: no gradient in the reference
    for k in names:
        gr = P[k].grad.reshape(-1)
        stride = int(g["gstride_" + k])
        ref = g["gsamp_" + k]
        assert rel_l2(gr[::stride][:2048], ref) < 1e-4, k
        assert abs(float(gr.double().norm()) - float(g["gnorm_" + k])) <= 1e-4 * float(g["gnorm_" + k]) + 1e-9, k


def test_ten_chained_blocks_vs_reference():
    """rollout10_sim: the reference's own 10 chained blocks (sim_inference.py:110-113, README.md:72 `--num_rollouts 10`;
    S = 10, B 1, T 8, L 4, full-width model).  The oracle chains ITS OWN end frames here (error carried over, as the product
    does).  Finding worth pinning: with seeded random weights the sampled structures are unphysical and the rollout glue
    (atom14 -> frames -> torsions, geometry.py:82-231) is ill-conditioned on them, so even fp32 summation-order noise
    (6e-6 A through block 1) is amplified to ~0.1 A max by block 2 and ~0.4 A max by block 9, while the rms stays ~1e-2 A.
    Chained-block parity can therefore only be gated on the first blocks and on the rms.  The masked entries of the glue's
    torsions' pre-omega angle of residue 0 (built from the zero padding) is pure rounding noise of the host and conditions the next
    block: that one entry is taken from tests/golden/host_rounding.npz, which records it as the chain produces it on the fixtures'
    host.  Every other torsion is the oracle's own."""
    g = load_golden("rollout10_sim")
    cfg, sd = weights_for(g)
    cd = O.cfg_dict(cfg)
    cur = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    seqres = cur["seqres"]
    S, T = 10, g["S10_b0_zs"].shape[1]
    pinned = load_golden("host_rounding")["rollout10_pre_omega0"]          # (10, B, 1, 2)
    assert (cur["torsion_mask"][:, 0, 0] == 0).all()
    for blk in range(10):
        ex = dict(cur)
        ex["torsions"] = cur["torsions"].expand(-1, T, -1, -1, -1)
        ex["trans"] = cur["trans"].expand(-1, T, -1, -1)
        ex["rots"] = cur["rots"].expand(-1, T, -1, -1, -1)
        atom14, aa, samples = O.inference(sd, cd, ex, g[f"S{S}_b{blk}_zs"], S)
        d = (atom14 - g[f"S{S}_b{blk}_atom14"]).abs()
        mx, rms = float(d.max()), float(d.pow(2).mean().sqrt())
        print(f"oracle chained on its own end frames, block {blk}: atom14 max {mx:.2e} A rms {rms:.2e} A")
        assert mx < (1e-4 if blk < 2 else 2.0) and rms < (1e-5 if blk < 2 else 0.05), blk
        cur = dict(cur, **O.rollout_glue(atom14[:, -1], seqres))
        cur["torsions"] = cur["torsions"].clone()
        cur["torsions"][:, :, 0, 0] = pinned[blk]


def _fp64_training_case(name):
    """Fixture `name` under compute_dtype float64: weights, inputs and the trainable leaves all fp64."""
    g = load_golden(name)
    cfg, sd = weights_for(g)
    from mdgen_amd.train import trainable_shapes
    names = list(trainable_shapes(cfg))
    P = {k: (v.double().requires_grad_(k in names) if v.is_floating_point() else v) for k, v in sd.items()}
    kw = dict(mask=g["mask"].double(), start_frames=(g["start_rot"].double(), g["start_trans"].double()),
              end_frames=(g["start_rot"].double(), g["start_trans"].double()), x_cond=g["x_cond"].double(),
              x_cond_mask=g["x_cond_mask"], aatype=g["aatype"])
    cd = dict(O.cfg_dict(cfg), compute_dtype="float64")
    args = (g["x1"].double(), g["loss_mask"].double(), kw, g["t"].double(), g["x0"].double())
    return g, names, P, cd, args


def test_fp64_mode_finite_differences():
    """compute_dtype float64 leaves no fp32 step in the training loss: along 3 random directions over every trainable
    tensor, the central difference (h = 1e-6) matches autograd's directional derivative to 1e-7 relative.  A single fp32
    step puts its rounding over h: the attention softmax alone left in fp32 gives 6e-4."""
    g, names, P, cd, args = _fp64_training_case("train_tiny_sim")
    with torch.enable_grad():
        out = O.training_losses(P, cd, *args)
        out["loss"].mean().backward()
    assert out["pred"].dtype == torch.float64 and out["loss"].dtype == torch.float64
    gen = torch.Generator().manual_seed(3)
    h = 1e-6
    for _ in range(3):
        v = {k: torch.randn(P[k].shape, generator=gen, dtype=torch.float64) for k in names}

        def f(s):
            Q = dict(P)
            for k in names:
                Q[k] = P[k].detach() + s * v[k]
            return float(O.training_losses(Q, cd, *args)["loss"].mean())

        fd = (f(h) - f(-h)) / (2 * h)
        ad = float(sum((P[k].grad * v[k]).sum() for k in names))
        assert abs(fd - ad) <= 1e-7 * abs(ad), (fd, ad)


def test_fp64_mode_gradients_vs_reference_autograd():
    """The fp64 oracle's gradients against the reference's own fp32 backward pass (train_grads_sim): the same gates as
    the fp32 oracle meets in test_training_gradients_vs_reference_autograd."""
    g, names, P, cd, args = _fp64_training_case("train_grads_sim")
    with torch.enable_grad():
        out = O.training_losses(P, cd, *args)
        out["loss"].mean().backward()
    assert torch.allclose(out["loss"].detach().float(), g["loss"], rtol=2e-5)
    assert sorted(names) == sorted(str(n) for n in g["grad_names"])
    for k in names:
        gr = P[k].grad.reshape(-1)
        assert gr.dtype == torch.float64, k
        ref = g["gsamp_" + k]
        assert rel_l2(gr[::int(g["gstride_" + k])][:2048], ref) < 1e-4, k
        assert abs(float(gr.norm()) - float(g["gnorm_" + k])) <= 1e-4 * float(g["gnorm_" + k]) + 1e-9, k
