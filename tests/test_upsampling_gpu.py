"""Trajectory upsampling on the GPU: `mdgen_prep_keyframes`, the fused `mdgen_upsample_euler` call behind
`NewMDGenWrapper.upsample`, and the sampler's parity with the CPU oracle when conditioning frames stand INSIDE the window
(every `cond_interval`-th frame), the pattern no other end-to-end test uses: the embed kernels' per-tile shortcuts (k_embed,
rows_embed_tail) meet tiles that mix conditioned and unconditioned rows here.

Gates are the project's existing ones: 5e-5 on the preparation (test_prep_batch_vs_reference), TOL_FWD / TOL_FP32 on a
forward, and the end-to-end triple of test_tps_inference_end_to_end_vs_oracle at the same size."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL_FWD, TOL_FP32 = 1e-2, 1e-5          # tests/test_gpu_parity.py
TOL_RMS_S3, TOL_MAX = 0.03, 0.5         # tol_rms(3), TOL_MAX of tests/test_gpu_parity.py
SEQS = ["FLRHA", "IMRYW", "AKDGS"]


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch.device("cuda")


def key_frames(B, T, L, c, seed):
    """Random self-consistent key frames (as the TPS end-to-end test builds its end states): frames + torsions -> atom14 with
    the oracle's geometry -> `get_batch_from_atom14`.  Returns (kb, wb): the key-frame batch (B,K,L,...) and the reference's
    window layout (B,T,L,...) -- zeros, identity rotations, key frames at [::c] -- both holding the ORACLE's values (CPU)."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import restype_order
    gen = torch.Generator().manual_seed(seed)
    K = -(-T // c)
    per = []
    for b in range(B):
        seqres = torch.tensor([restype_order[ch] for ch in SEQS[b % len(SEQS)][:L]])
        assert seqres.shape[0] == L
        q = torch.randn(1, K, L, 4, generator=gen)
        R = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
        tr = torch.cumsum(2.2 * torch.randn(1, K, L, 3, generator=gen), 2)
        ang = torch.randn(1, K, L, 7, 2, generator=gen)
        ang = ang / ang.norm(dim=-1, keepdim=True)
        a14 = O.frames_torsions_to_atom14(R, tr, ang, seqres[None, None].expand(1, K, L))[0]   # [K,L,14,3]
        ob = O.get_batch_from_atom14(a14, seqres)
        per.append({k: v.float() if v.is_floating_point() else v for k, v in ob.items()})
    kb = {k: torch.stack([p[k] for p in per], 0) for k in per[0]}
    wb = {"torsions": torch.zeros(B, T, L, 7, 2), "trans": torch.zeros(B, T, L, 3),
          "rots": torch.eye(3).expand(B, T, L, 3, 3).clone(), "torsion_mask": kb["torsion_mask"], "seqres": kb["seqres"],
          "mask": kb["mask"]}
    for k in ("torsions", "trans", "rots"):
        wb[k][:, ::c] = kb[k]
    return kb, wb


def to_dev(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def make_wrapper(T, c, seed=9, precision="bf16", L=4):
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper, default_args
    cfg = ModelConfig.forward_sim(num_frames=T, crop=max(L, 4))
    args = default_args(cfg)
    args.cond_interval = c
    w = NewMDGenWrapper(args, precision=precision)
    sd = synth_state_dict(cfg, seed)
    w.model.load_state_dict(sd)
    return w, cfg, sd


@functools.lru_cache(maxsize=None)
def case_2_12_4():
    """The shape of tests 2-5: B = 2 windows of T = 12 frames, L = 4, key frames every c = 4, S = 3 steps; built once."""
    B, T, L, c = 2, 12, 4, 4
    kb, wb = key_frames(B, T, L, c, 77)
    zs = torch.randn(B, T, L, 21, generator=torch.Generator().manual_seed(78))
    return B, T, L, c, 3, kb, wb, zs


def manual_chain(w, kb, zs, T, c, S, use_graph):
    """prep_keyframes -> model.sample_euler -> samples_to_atom14: the fused call's three steps as three calls."""
    from mdgen_amd.geometry import prep_keyframes, samples_to_atom14
    B, _, L = kb["trans"].shape[:3]
    p = prep_keyframes(kb["rots"], kb["trans"], kb["torsions"], T, c)
    mask = kb["mask"].float()[:, None].expand(B, T, L).contiguous()
    samples = w.model.sample_euler(zs, S, mask=mask, start_frames=(p["start_rot"], p["start_trans"]), x_cond=p["x_cond"],
                                   x_cond_mask=p["x_cond_mask"], aatype=kb["seqres"], use_graph=use_graph)
    return samples_to_atom14(samples, p["start_rot"], p["start_trans"], kb["seqres"], False), samples


# ---- test 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 10, 5, 3), (1, 8, 4, 1), (2, 6, 4, 6), (1, 7, 3, 9), (3, 12, 4, 4)])
def test_prep_keyframes_vs_prep_latents_and_oracle(shape):
    """`mdgen_prep_keyframes` alone: T no multiple of c (K = 4); every frame a key frame; c = T (K = 1); c > T; three
    windows.  Against `mdgen_prep_latents(..., cond_interval = c)` on the scattered window and against the oracle's
    `prep_batch`: mask equal, non-key rows exactly zero, key rows within 5e-5, start frames = key frame 0."""
    from oracle import mdgen_oracle as O
    import mdgen_amd._lib as L_
    from mdgen_amd.geometry import prep_keyframes
    dev = _cuda()
    B, T, L, c = shape
    K = -(-T // c)
    kb, wb = key_frames(B, T, L, c, 100 + 7 * T + c)
    assert kb["trans"].shape == (B, K, L, 3)
    d = to_dev(kb, dev)
    got = prep_keyframes(d["rots"], d["trans"], d["torsions"], T, c)
    # the existing kernel on the reference's window layout
    wd = to_dev(wb, dev)
    lat = torch.empty(B, T, L, 21, device=dev)
    xc = torch.empty(B, T, L, 21, device=dev)
    cm = torch.empty(B, T, L, dtype=torch.int64, device=dev)
    sh = L_.Shape(B, T, L)
    L_.launch(L_.lib.mdgen_prep_latents, lat, C.byref(sh), 0, c, L_.ptr(wd["rots"].contiguous()),
              L_.ptr(wd["trans"].contiguous()), L_.ptr(wd["torsions"].contiguous()), L_.ptr(lat), L_.ptr(xc), L_.ptr(cm))
    torch.cuda.synchronize()
    ref = O.prep_batch(wb, dict(sim_condition=True, cond_interval=c))["model_kwargs"]
    want_mask = torch.zeros(B, T, L, dtype=torch.long)
    want_mask[:, ::c] = 1
    print(f"{shape}: k_prep_keyframes == k_prep_latents bit for bit: x_cond {torch.equal(got['x_cond'], xc)}, "
          f"max |x_cond - oracle| {float((got['x_cond'].cpu() - ref['x_cond']).abs().max()):.2e}")
    assert got["x_cond_mask"].dtype == torch.int64
    assert torch.equal(got["x_cond_mask"].cpu(), want_mask)
    assert torch.equal(got["x_cond_mask"], cm) and torch.equal(ref["x_cond_mask"], want_mask)
    nonkey = want_mask == 0
    assert torch.equal(got["x_cond"].cpu()[nonkey], torch.zeros(int(nonkey.sum()), 21))
    assert torch.allclose(got["x_cond"], xc, atol=5e-5)
    assert torch.allclose(got["x_cond"].cpu(), ref["x_cond"], atol=5e-5)
    assert torch.equal(got["start_rot"].cpu(), kb["rots"][:, 0]) and torch.equal(got["start_trans"].cpu(), kb["trans"][:, 0])
    assert got["start_rot"].is_contiguous() and got["start_trans"].is_contiguous()
    # one device function computes the offsets of both kernels
    assert torch.equal(got["x_cond"], xc)


# ---- test 2 ----------------------------------------------------------------------------------------------------------
def test_fused_upsample_is_the_sum_of_its_parts():
    """`wrapper.upsample` (one `mdgen_upsample_euler` call) against prep_keyframes -> sample_euler -> samples_to_atom14 on
    the same noise: samples and atom14 bitwise equal, eager and graph; again with option "streams" = 2 set explicitly.
    (At this size, 96 tokens, the sampler keeps one stream whatever the option says -- n_streams() needs 4096 tokens; the
    forked schedule is covered by test_fused_upsample_on_two_sub_batch_streams.)"""
    dev = _cuda()
    B, T, L, c, S, kb, wb, zs = case_2_12_4()
    w, cfg, sd = make_wrapper(T, c)
    d, z = to_dev(kb, dev), zs.to(dev)
    ref14, ref_s = manual_chain(w, d, z, T, c, S, use_graph=False)
    assert torch.isfinite(ref14).all()
    for streams in (None, 2):
        if streams is not None:
            w.model.set_option("streams", streams)
        for use_graph in (False, True, True):
            a14, aa = w.upsample(d, zs=z, num_steps=S, use_graph=use_graph)
            torch.cuda.synchronize()
            assert a14.shape == (B, T, L, 14, 3) and aa.shape == (B, T, L)
            assert torch.equal(aa, d["seqres"][:, None].expand(B, T, L))
            assert torch.equal(w.last_samples, ref_s), (streams, use_graph)
            assert torch.equal(a14, ref14), (streams, use_graph)
        m14, m_s = manual_chain(w, d, z, T, c, S, use_graph=True)
        assert torch.equal(m_s, ref_s) and torch.equal(m14, ref14)


def test_fused_upsample_on_two_sub_batch_streams():
    """The smallest size at which the Euler loop really forks (n_streams(): 4096 tokens, option "streams" = 2 set
    explicitly): B = 2 windows of 512 frames, L = 4, key frames every 128.  The preparation kernel is enqueued before the
    fork, so the second stream's sample must see THIS call's conditioning: fused call == manual chain bitwise, for key
    frames A, then B, then A again through the same staging buffers and the same graph."""
    import mdgen_amd._lib as L_
    dev = _cuda()
    B, T, L, c, S = 2, 512, 4, 128, 2
    assert L_.dispatch_plan(B, T, L, n_steps=S, options={"streams": 2})["streams"] == 2
    w, cfg, sd = make_wrapper(T, c)
    w.model.set_option("streams", 2)
    kbA, _ = key_frames(B, T, L, c, 31)
    kbB, _ = key_frames(B, T, L, c, 32)
    z = torch.randn(B, T, L, 21, generator=torch.Generator().manual_seed(33)).to(dev)
    refs = {}
    for tag, kb in (("A", kbA), ("B", kbB)):
        refs[tag] = manual_chain(w, to_dev(kb, dev), z, T, c, S, use_graph=False)
    assert not torch.equal(refs["A"][1], refs["B"][1])
    for use_graph in (True, False):
        for tag, kb in (("A", kbA), ("B", kbB), ("A", kbA)):
            a14, _ = w.upsample(to_dev(kb, dev), zs=z, num_steps=S, use_graph=use_graph)
            torch.cuda.synchronize()
            assert torch.equal(w.last_samples, refs[tag][1]), (use_graph, tag)
            assert torch.equal(a14, refs[tag][0]), (use_graph, tag)


# ---- test 3 ----------------------------------------------------------------------------------------------------------
def test_graph_replay_sees_new_key_frames():
    """upsample(use_graph=True) with key frames A, B, A: same staging buffers, same graph (the preparation kernel is part
    of it).  A's results equal each other and the eager result bitwise; B's differ from A's."""
    dev = _cuda()
    B, T, L, c, S, kbA, _, zs = case_2_12_4()
    kbB, _ = key_frames(B, T, L, c, 177)
    w, cfg, sd = make_wrapper(T, c)
    z = zs.to(dev)
    dA, dB = to_dev(kbA, dev), to_dev(kbB, dev)
    eagerA, _ = w.upsample(dA, zs=z, num_steps=S, use_graph=False)
    eagerA_s = w.last_samples
    eagerB, _ = w.upsample(dB, zs=z, num_steps=S, use_graph=False)
    outs = []
    for d in (dA, dB, dA):
        a14, _ = w.upsample(d, zs=z, num_steps=S, use_graph=True)
        outs.append((a14, w.last_samples))
    torch.cuda.synchronize()
    assert len(w.model._stage) == 1          # one set of staging buffers served all five calls
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    assert torch.equal(outs[0][0], eagerA) and torch.equal(outs[0][1], eagerA_s)
    assert torch.equal(outs[1][0], eagerB)
    assert not torch.equal(outs[1][1], outs[0][1]) and not torch.equal(outs[1][0], outs[0][0])


# ---- test 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_forward_parity_with_mixed_conditioning_tiles(precision):
    """`model.forward` with the key-frame x_cond / x_cond_mask (conditioned rows at t = 0, 4, 8 of 12: every 64-row tile of
    the embed kernels mixes conditioned and unconditioned rows) against the oracle; the h0 trace localises an embedding
    fault.  Gates: the project's forward gates, rel-L2 < 1e-2 (bf16 operands) / < 1e-5 (precision 32)."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import prep_keyframes
    dev = _cuda()
    B, T, L, c, S, kb, wb, _ = case_2_12_4()
    w, cfg, sd = make_wrapper(T, c, precision=precision)
    prep = O.prep_batch(wb, dict(O.cfg_dict(cfg), cond_interval=c))["model_kwargs"]
    gen = torch.Generator().manual_seed(79)
    x = torch.randn(B, T, L, 21, generator=gen)
    t = torch.rand(B, generator=gen)
    kw = dict(x=x, t=t, mask=prep["mask"].contiguous(), start_frames=prep["start_frames"], end_frames=prep["end_frames"],
              x_cond=prep["x_cond"], x_cond_mask=prep["x_cond_mask"], aatype=prep["aatype"])
    ref, rtr = O.forward(sd, O.cfg_dict(cfg), return_trace=True, **kw)
    assert int(prep["x_cond_mask"].sum()) == B * 3 * L and float(prep["x_cond"][:, 4].abs().max()) > 0
    dkw = {k: (tuple(u.to(dev) for u in v) if isinstance(v, tuple) else v.to(dev)) for k, v in kw.items()}
    # the device's own preparation feeds the same forward: its x_cond is the oracle's to 5e-5 (test 1)
    d = to_dev(kb, dev)
    own = prep_keyframes(d["rots"], d["trans"], d["torsions"], T, c)
    assert torch.allclose(own["x_cond"].cpu(), prep["x_cond"], atol=5e-5)
    out, tr = w.model.forward(**dkw, return_trace=True)
    torch.cuda.synchronize()
    tol = TOL_FWD if precision == "bf16" else TOL_FP32
    rep = {"h0": rel_l2(tr["h0"].cpu(), rtr["h0"]), "ipa_out": rel_l2(tr["ipa_out"].cpu(), rtr["ipa_out"]),
           f"h{cfg.num_layers}": rel_l2(tr[f"h{cfg.num_layers}"].cpu(), rtr[f"h{cfg.num_layers}"]),
           "out": rel_l2(out.cpu(), ref)}
    # per-row h0 error, conditioned rows and the others apart
    e = (tr["h0"].cpu().double() - rtr["h0"].double()).norm(dim=-1) / rtr["h0"].double().norm(dim=-1)
    km = prep["x_cond_mask"].bool()
    print(f"key-frame forward ({precision}):", {k: f"{v:.2e}" for k, v in rep.items()},
          f"h0 worst row: key {float(e[km].max()):.2e}, other {float(e[~km].max()):.2e}")
    assert torch.isfinite(out).all()
    for k, v in rep.items():
        assert v < tol, (k, v)


# ---- test 5 ----------------------------------------------------------------------------------------------------------
def test_upsample_end_to_end_vs_oracle():
    """`wrapper.upsample` against the oracle's `inference` on the reference's window layout with `cond_interval`: B = 2,
    T = 12, L = 4, c = 4, S = 3; gates of the TPS end-to-end test at this size (samples rel-L2 < 2e-2, atom14 rms < 0.03 A,
    max < 0.5 A).  The frame-0-only pattern (c = T) runs beside it on the same weights and noise."""
    from oracle import mdgen_oracle as O
    dev = _cuda()
    B, T, L, c, S, kb, wb, zs = case_2_12_4()
    rep = {}
    for tag, ci in (("key frames", c), ("frame 0 only", T)):
        w, cfg, sd = make_wrapper(T, ci)
        K = -(-T // ci)
        kbi = {k: (v[:, :K] if k in ("torsions", "trans", "rots") else v) for k, v in kb.items()}
        wbi = dict(wb)
        if ci == T:   # the window that holds key frame 0 alone
            for k, fill in (("torsions", 0.0), ("trans", 0.0)):
                wbi[k] = wb[k].clone()
                wbi[k][:, 1:] = fill
            wbi["rots"] = wb["rots"].clone()
            wbi["rots"][:, 1:] = torch.eye(3)
        a14, _ = w.upsample(to_dev(kbi, dev), zs=zs.to(dev), num_steps=S, use_graph=False)
        torch.cuda.synchronize()
        ref14, _, ref_s = O.inference(sd, dict(O.cfg_dict(cfg), cond_interval=ci), wbi, zs, S)
        d = (a14.cpu() - ref14).abs()
        rep[tag] = (rel_l2(w.last_samples.cpu(), ref_s), float(d.pow(2).mean().sqrt()), float(d.max()), ref_s, ref14)
        assert torch.isfinite(a14).all()
        print(f"upsampling end-to-end S={S}, {tag} (c = {ci}): samples rel-L2 {rep[tag][0]:.2e}  atom14 rms "
              f"{rep[tag][1]:.4f} A max {rep[tag][2]:.4f} A")
    dd = (rep["key frames"][4] - rep["frame 0 only"][4]).abs()
    print(f"oracle with key frames vs oracle without: samples rel-L2 {rel_l2(rep['frame 0 only'][3], rep['key frames'][3]):.2e}  "
          f"atom14 rms {float(dd.pow(2).mean().sqrt()):.3f} A max {float(dd.max()):.2f} A")
    for tag in rep:
        e_s, rms, mx = rep[tag][:3]
        assert e_s < 2e-2, (tag, e_s)
        assert rms < TOL_RMS_S3 and mx < TOL_MAX, (tag, rms, mx)


# ---- test 6 ----------------------------------------------------------------------------------------------------------
def test_upsample_dopri5_route():
    """upsample(sampling_method="dopri5") = prep_keyframes -> sample_dopri5 -> samples_to_atom14 equals
    inference(window batch, sampling_method="dopri5") bitwise (two runs of the solver on the same inputs are bitwise equal,
    tests/test_ode_gpu.py; the two preparations agree bit for bit, test 1); the solver's counts land in last_stats."""
    from mdgen_amd._lib import MdgenError
    dev = _cuda()
    B, T, L, c = 1, 8, 4, 4
    kb, wb = key_frames(B, T, L, c, 61)
    w, cfg, sd = make_wrapper(T, c)
    z = torch.randn(B, T, L, 21, generator=torch.Generator().manual_seed(62)).to(dev)
    a_up, _ = w.upsample(to_dev(kb, dev), zs=z, sampling_method="dopri5")
    s_up, st_up = w.last_samples.clone(), dict(w.last_stats)
    a_inf, _ = w.inference(to_dev(wb, dev), zs=z, sampling_method="dopri5")
    torch.cuda.synchronize()
    print(f"dopri5 upsample: nfe {st_up['nfe']} ({st_up['accepted']} accepted / {st_up['rejected']} rejected)")
    assert st_up["nfe"] > 0 and st_up["accepted"] > 0 and len(st_up["steps"]) == st_up["accepted"]
    assert st_up == w.last_stats
    assert torch.isfinite(a_up).all()
    assert torch.equal(s_up, w.last_samples) and torch.equal(a_up, a_inf)
    with pytest.raises(MdgenError):   # the Euler grid and the adaptive solver exclude each other
        w.upsample(to_dev(kb, dev), zs=z, sampling_method="dopri5", num_steps=3)


def test_upsample_refuses_what_it_cannot_run():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.wrapper import NewMDGenWrapper, default_args
    dev = _cuda()
    B, T, L, c = 1, 8, 4, 4
    kb, _ = key_frames(B, T, L, c, 61)
    d = to_dev(kb, dev)
    w, cfg, sd = make_wrapper(T, c)
    with pytest.raises(MdgenError, match="key frames"):          # K != ceil(T / c)
        w.upsample(d, num_frames=12, num_steps=2)
    w.args.sampling_method = "dopri5"                            # a checkpoint whose args name the adaptive solver
    with pytest.raises(MdgenError, match="sampling_method"):
        w.upsample(d)
    plain = NewMDGenWrapper(default_args(ModelConfig.forward_sim(num_frames=T)))
    with pytest.raises(MdgenError, match="cond_interval"):
        plain.upsample(d, num_steps=2)
    with pytest.raises(MdgenError):                              # ... and rollout() still refuses cond_interval models
        w.rollout(d, T, 1, num_steps=2)
    targs = default_args(ModelConfig.tps(num_frames=T))
    targs.cond_interval = c
    with pytest.raises(MdgenError, match="two-sided"):
        NewMDGenWrapper(targs).upsample(d, num_steps=2)


# ---- test 7 ----------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path):
    """`python -m mdgen_amd.upsampling_inference` in-process: 7 key frames, T = 12, c = 4 -> two windows of three key frames,
    one key frame dropped; two names, one of them listed twice under --pdb_id."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import restype_order
    from mdgen_amd.upsampling_inference import main
    _cuda()
    data, out = tmp_path / "data", tmp_path / "out"
    data.mkdir()
    names = {"pA": "FLRH", "pB": "IMRY"}
    gen = torch.Generator().manual_seed(5)
    for n, sq in names.items():
        seqres = torch.tensor([restype_order[ch] for ch in sq])
        q = torch.randn(1, 7, 4, 4, generator=gen)
        tr = torch.cumsum(2.2 * torch.randn(1, 7, 4, 3, generator=gen), 2)
        ang = torch.randn(1, 7, 4, 7, 2, generator=gen)
        a14 = O.frames_torsions_to_atom14(O.quat_to_rot(q / q.norm(dim=-1, keepdim=True)), tr,
                                          ang / ang.norm(dim=-1, keepdim=True), seqres[None, None].expand(1, 7, 4))[0]
        np.save(data / f"{n}_i100.npy", a14.numpy().astype(np.float32))
    (tmp_path / "split.csv").write_text("name,seqres\n" + "".join(f"{n},{s}\n" for n, s in names.items()))
    res = main(["--synthetic", "--num_frames", "12", "--cond_interval", "4", "--batch_size", "2", "--num_steps", "3", "--npy",
                "--data_dir", str(data), "--split", str(tmp_path / "split.csv"), "--out_dir", str(out),
                "--pdb_id", "pA", "pB", "pA"])
    assert res["names"] == ["pA", "pB"] and res["frames"] == 48
    for n in names:
        arr = np.load(out / f"{n}.npy")
        assert arr.shape == (24, 4, 14, 3) and np.isfinite(arr).all()
        assert open(out / f"{n}.pdb").read().count("MODEL") == 24
    assert sorted(os.listdir(out)) == ["pA.npy", "pA.pdb", "pB.npy", "pB.pdb"]
