"""The fixed-grid Runge-Kutta samplers on the GPU (mdgen_sample_rk: csrc/ode.inc + csrc/k_rk.hip) against tests/rk_ref.py -- the
torch restatement of torchdiffeq 0.2.x's midpoint / heun3 / rk4 -- : the state-forming embedding kernel alone against fp64, the
whole solve against the CPU oracle's forward and against a host loop over the library's own forward, the bf16 path, capture and
determinism, batch independence and the CLI."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rk_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
METHODS = list(R.METHODS)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch.device("cuda")


def _model_kwargs(w, batch):
    kw = dict(w.prep_batch(batch)["model_kwargs"])
    kw["mask"] = kw["mask"].contiguous()
    if not w.args.tps_condition:
        kw["end_frames"] = None
    return kw


def _wrapper(B, T, L_, tps=False, abs_pos=True, n_pad=0, precision="fp32", wseed=9, bseed=31, zseed=5):
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_batch, synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper
    dev = _cuda()
    cfg = ModelConfig(crop=L_, num_frames=T, abs_pos_emb=abs_pos, sim_condition=not tps, tps_condition=tps)
    sd = synth_state_dict(cfg, wseed)
    w = NewMDGenWrapper(cfg, device=dev, precision=precision)
    w.model.load_state_dict(sd)
    batch = synth_batch(B, T, L_, n_pad, dev, seed=bseed, tps=tps)
    zs = torch.randn(B, T, L_, cfg.latent_dim, generator=torch.Generator().manual_seed(zseed))
    return w, sd, cfg, batch, zs


# ---- 5: k_rk_embed alone --------------------------------------------------------------------------------------------------------
# h: the metric and the gate of tests/ipa_ref.py -- (largest row error / rms row norm, rel-L2) against fp64, gated at 32 x what
# torch's own fp32 evaluation of the same expression shows (and at least 32 fp32 ulps).  Stored state: elementwise
# |got - fp64| <= 4 * 2^-23 * (|y0| + |dt| sum_j |c_j k_j|), a forward bound for at most six rounded operations; the kernel's
# operations are also rk_ref's fp32 operations one by one, so the state equals rk_ref's fp32 value bit for bit.
FACTOR, ULPS = 32.0, 32.0 * 2.0 ** -24
STAGE_SHAPES = [(1, 5, 3), (3, 11, 4), (5, 999, 10)]
DT = float(np.float32(1.0) / np.float32(12.0))


@functools.lru_cache(maxsize=None)
def _embed_model(tps, abs_pos, crop):
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.model import LatentMDGenModel
    from mdgen_amd.synthetic import synth_state_dict
    cfg = ModelConfig(num_layers=1, crop=crop, num_frames=8, abs_pos_emb=abs_pos, sim_condition=not tps, tps_condition=tps)
    sd = synth_state_dict(cfg, 4)
    m = LatentMDGenModel(cfg, _cuda())
    m.load_state_dict(sd)
    return m, sd


def _rows(dev, ref):
    dev, ref = dev.double(), ref.double()
    scale = float(ref.norm(dim=-1).pow(2).mean().sqrt().clamp_min(1e-300))
    e = (dev - ref).norm(dim=-1)
    return float(e.max() / scale), float(e.norm() / ref.norm().clamp_min(1e-300))


def _embedding(sd, x, x_cond, xcm, ipa_out, abs_pos, dtype, dev="cpu"):
    """latent_to_emb(x) + cond_to_emb(x_cond) + mask_to_emb[x_cond_mask] + pos_embed + ipa_out (latent_model.py:233-246), evaluated
    by torch in `dtype` on `dev`."""
    P = {k: sd[k].to(device=dev, dtype=dtype) for k in ("latent_to_emb.weight", "latent_to_emb.bias", "cond_to_emb.weight",
                                                         "cond_to_emb.bias", "mask_to_emb.weight")}
    B, T, L_, _ = x.shape
    h = x.to(device=dev, dtype=dtype) @ P["latent_to_emb.weight"].T + P["latent_to_emb.bias"]
    h = h + (x_cond.to(device=dev, dtype=dtype) @ P["cond_to_emb.weight"].T + P["cond_to_emb.bias"])
    h = h + P["mask_to_emb.weight"][xcm.to(dev)]
    if abs_pos:
        h = h + sd["pos_embed"].to(device=dev, dtype=dtype)[:, :L_]
    if ipa_out is not None:
        h = h + ipa_out.to(device=dev, dtype=dtype).view(B, 1, L_, -1)
    return h.reshape(B * T * L_, -1)


def _cond_pattern(kind, B, T, L_, D, gen):
    """x_cond, x_cond_mask.  "frame0": frame 0 of every sample, as the samplers set it.  "tiles": tokens of every third 32-token
    tile, which leaves whole tiles unconditioned (the kernel skips cond_to_emb there), plus a few tokens with the mask set on a
    zero x_cond row and a few with values but no mask (the two are independent inputs)."""
    N = B * T * L_
    x_cond = torch.zeros(N, D)
    xcm = torch.zeros(N, dtype=torch.int64)
    tok = torch.arange(N)
    if kind == "frame0":
        sel = (tok // L_) % T == 0
        x_cond[sel] = torch.randn(int(sel.sum()), D, generator=gen)
        xcm[sel] = 1
    else:
        sel = (tok // 32) % 3 == 1 if N > 32 else tok % 4 == 1
        x_cond[sel] = torch.randn(int(sel.sum()), D, generator=gen)
        xcm[sel] = 1
        xcm[tok % 37 == 5] = 1
        loose = tok % 41 == 7
        x_cond[loose] = torch.randn(int(loose.sum()), D, generator=gen)
    return x_cond.view(B, T, L_, D), xcm.view(B, T, L_)


@pytest.mark.parametrize("abs_pos", [True, False])
@pytest.mark.parametrize("tps", [False, True])
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_rk_embed_kernel_vs_fp64(shape, tps, abs_pos):
    from mdgen_amd import _lib as L
    dev = _cuda()
    B, T, L_ = shape
    model, sd = _embed_model(tps, abs_pos, L_)
    D = model.cfg.latent_dim
    N = B * T * L_
    gen = torch.Generator().manual_seed(1000 * B + L_)
    y0 = torch.randn(B, T, L_, D, generator=gen)
    k = [torch.randn(B, T, L_, D, generator=gen) * s for s in (3.0, 0.5, 7.0, 1.5)]
    ipa = torch.randn(B * L_, 384, generator=gen)
    dt = torch.tensor(DT, dtype=torch.float32)
    # the large shape pairs the switches (two combinations); the small ones take all four
    combos = [(True, "frame0"), (False, "tiles")] if N > 10000 else [(i, c) for i in (True, False) for c in ("frame0", "tiles")]
    sh = L.Shape(B, T, L_)
    k_dev = [a.to(dev) for a in k]
    worst = (0.0, 0.0)
    for with_ipa, kind in combos:
        x_cond, xcm = _cond_pattern(kind, B, T, L_, D, gen)
        xc_dev, xcm_dev = x_cond.to(dev), xcm.to(dev)
        ipa_dev = ipa.to(dev) if with_ipa else None
        for method in METHODS:
            for stage in range(R.STAGES[method] + 1):
                storing = stage == R.STAGES[method]
                x64 = R.state(method, stage, y0.double(), [a.double() for a in k], dt.double())
                x32 = R.state(method, stage, y0, k, dt)
                # the fp64 reference on the device (its rounding is far below every fp32 effect); torch's fp32 evaluation on the CPU
                ref = _embedding(sd, x64, x_cond, xcm, ipa if with_ipa else None, abs_pos, torch.float64, dev)
                floor = _rows(_embedding(sd, x32, x_cond, xcm, ipa if with_ipa else None, abs_pos, torch.float32).to(dev), ref)
                y_dev = y0.to(dev)
                h = torch.full((N, 384), float("nan"), device=dev)
                with torch.cuda.device(dev):
                    L.check(L.lib.mdgen_debug_rk_stage(model._ctx, C.byref(sh), R.METHODS[method], stage, DT, L.ptr(y_dev),
                                                       *[L.ptr(a) for a in k_dev], L.ptr(xc_dev), L.ptr(xcm_dev), L.ptr(ipa_dev),
                                                       L.ptr(h), L.stream_ptr()))
                got = _rows(h, ref)
                gate = tuple(max(FACTOR * f, ULPS) for f in floor)
                worst = max(worst, (got[0] / max(floor[0], 1e-30), got[1] / max(floor[1], 1e-30)))
                tag = (shape, tps, abs_pos, with_ipa, kind, method, stage)
                assert torch.isfinite(h).all(), tag
                assert got[0] <= gate[0] and got[1] <= gate[1], (tag, got, gate)
                if storing:   # y1 over y0
                    cw = R.weights(method, stage)
                    bound = 4 * 2.0 ** -23 * (y0.double().abs() + abs(DT) * sum(abs(c) * a.double().abs() for c, a in zip(cw, k)))
                    err = (y_dev.cpu().double() - x64).abs()
                    assert bool((err <= bound).all()), (tag, float((err / bound).max()))
                    assert torch.equal(y_dev.cpu(), x32), tag
                else:         # a stage input exists only inside the launch
                    assert torch.equal(y_dev.cpu(), y0), tag
    print(f"{shape} D {D} pos {abs_pos}: worst h error / fp32 floor: row max x{worst[0]:.2f}, rel-L2 x{worst[1]:.2f} (gate x{FACTOR:.0f})")


# ---- 5b: one embedding body -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abs_pos", [True, False])
@pytest.mark.parametrize("tps", [False, True])
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_embed_kernels_share_one_body_bit_for_bit(shape, tps, abs_pos):
    """k_embed, k_rk_embed on the state y0 itself and k_sde_embed on the state x itself are one device body (csrc/state_embed.h): on
    the same inputs the three write the same h bit for bit, and none of them touches x.  The shapes are a partial 32-token tile,
    132 tokens (32-token workgroups, partial last one) and 49 950 tokens (just past the 384 x 128 threshold: 128-token workgroups,
    partial last one); "tiles" leaves whole tiles unconditioned, so the cond_to_emb skip runs in all three."""
    import sde_ref
    from mdgen_amd import _lib as L
    from mdgen_amd.synthetic import synth_forward_inputs
    dev = _cuda()
    B, T, L_ = shape
    model, _ = _embed_model(tps, abs_pos, L_)
    D = model.cfg.latent_dim
    N = B * T * L_
    inp = synth_forward_inputs(model.cfg, B, T, L_, 0, 3000 * B + L_)
    gen = torch.Generator().manual_seed(3000 * B + L_)
    x = inp["x"].to(dev)
    sh = L.Shape(B, T, L_)
    o = L.sde_opts("Euler", "GVP", "sigma", 1.0, "Mean", 0.04, 6, 0.0)
    for kind in ("frame0", "tiles"):
        x_cond, xcm = _cond_pattern(kind, B, T, L_, D, gen)
        xc_dev, xcm_dev = x_cond.to(dev), xcm.to(dev)
        x_fwd = x.clone()
        _, tr = model.forward(x=x_fwd, t=inp["t"].to(dev), mask=inp["mask"].to(dev),
                              start_frames=(inp["start_rot"].to(dev), inp["start_trans"].to(dev)),
                              end_frames=(inp["end_rot"].to(dev), inp["end_trans"].to(dev)) if tps else None,
                              x_cond=xc_dev, x_cond_mask=xcm_dev, aatype=inp["aatype"].to(dev), return_trace=True)
        h_embed = tr["h0"].reshape(N, 384)
        ipa_dev = tr["ipa_out"].reshape(B * L_, 384).contiguous()
        x_rk, x_sde = x.clone(), x.clone()
        h_rk = torch.full((N, 384), float("nan"), device=dev)
        h_sde = torch.full((N, 384), float("nan"), device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib.mdgen_debug_rk_stage(model._ctx, C.byref(sh), R.METHODS["rk4"], 0, DT, L.ptr(x_rk), None, None, None, None,
                                               L.ptr(xc_dev), L.ptr(xcm_dev), L.ptr(ipa_dev), L.ptr(h_rk), L.stream_ptr()))
            L.check(L.lib.mdgen_debug_sde_stage(model._ctx, C.byref(sh), C.byref(o), sde_ref.X, 0, L.ptr(x_sde), None, None, None,
                                                L.ptr(xc_dev), L.ptr(xcm_dev), L.ptr(ipa_dev), L.ptr(h_sde), L.stream_ptr()))
        torch.cuda.synchronize()
        tag = (shape, tps, abs_pos, kind)
        assert torch.isfinite(h_embed).all(), tag
        assert torch.equal(h_rk, h_embed), (tag, "k_rk_embed", float((h_rk - h_embed).abs().max()))
        assert torch.equal(h_sde, h_embed), (tag, "k_sde_embed", float((h_sde - h_embed).abs().max()))
        assert torch.equal(x_fwd, x) and torch.equal(x_rk, x) and torch.equal(x_sde, x), tag


# ---- 6: whole solve, fp32 mode, against the oracle ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_setup(tps):
    from oracle import mdgen_oracle as O
    B, T, L_ = 2, 12, 4
    w, sd, cfg, batch, zs = _wrapper(B, T, L_, tps=tps)
    obatch = {k: v.cpu() for k, v in batch.items()}
    c = dict(O.cfg_dict(cfg), quat_sign="w_nonneg") if tps else O.cfg_dict(cfg)
    prep = O.prep_batch(obatch, c)
    return w, sd, c, batch, obatch, prep, zs


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("tps", [False, True])
def test_rk_fp32_vs_oracle(tps, method):
    from oracle import mdgen_oracle as O
    w, sd, c, batch, obatch, prep, zs = _oracle_setup(tps)
    B, S = zs.shape[0], 3
    atom14, _ = w.inference(batch, zs=zs.to(w.device), sampling_method=method, num_steps=S)
    mk = prep["model_kwargs"]
    ref = R.solve(lambda t, y: O.forward(sd, c, y, torch.ones(B) * t, **mk), zs, method, S)
    e = rel_l2(w.last_samples.cpu(), ref)
    d = float((atom14.cpu() - O.postprocess(ref, prep["rigids"], obatch["seqres"], c)[0]).abs().max())
    print(f"tps={tps} {method} S={S}: samples rel-L2 {e:.2e}, atom14 max {d:.2e} A")
    assert e <= 1e-5 and d <= 1e-3


# ---- 7: whole solve against the host loop over the library's own forward -----------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["B2_T12_L4", "B3_T40_L5_pad2_nopos"])
def test_rk_vs_host_loop_over_library_forward(case, method):
    B, T, L_, abs_pos, n_pad = {"B2_T12_L4": (2, 12, 4, True, 0), "B3_T40_L5_pad2_nopos": (3, 40, 5, False, 2)}[case]
    w, _, _, batch, zs = _wrapper(B, T, L_, abs_pos=abs_pos, n_pad=n_pad, wseed=0, bseed=100, zseed=137)
    dev = w.device
    zs = zs.to(dev)
    kw = _model_kwargs(w, batch)
    S = 3
    x = w.model.sample_rk(zs, method, S, **kw)
    ref = R.solve(lambda t, y: w.model.forward(y, torch.ones(B, device=dev) * t, **kw), zs, method, S)
    e = rel_l2(x, ref)
    print(f"{case} {method} S={S}: rel-L2 against the host loop {e:.2e}")
    assert e <= 1e-5


# ---- 8: bf16 path against fp32 mode -----------------------------------------------------------------------------------------------
def test_rk4_bf16_vs_fp32_mode():
    w, _, _, batch, zs = _wrapper(2, 12, 4)
    zs = zs.to(w.device)
    a32, _ = w.inference(batch, zs=zs, sampling_method="rk4", num_steps=12)
    s32 = w.last_samples.clone()
    w.model.set_precision("bf16")
    a16, _ = w.inference(batch, zs=zs, sampling_method="rk4", num_steps=12)
    s16 = w.last_samples.clone()
    m = batch["mask"][:, None, :, None, None].bool()
    d = (a16 - a32).masked_select(m.expand_as(a16))
    e, rms = rel_l2(s16, s32), float(d.pow(2).mean().sqrt())
    print(f"rk4 S=12 bf16 against fp32 mode: samples rel-L2 {e:.2e}, atom14 rms {rms:.4f} A")
    assert torch.isfinite(a16).all() and torch.isfinite(s16).all()
    assert e <= 1e-2 and rms <= 0.02


# ---- 9: capture and determinism -----------------------------------------------------------------------------------------------
def test_rk_graph_replay_is_deterministic_and_equals_the_direct_run():
    w, _, _, batch, zs = _wrapper(2, 12, 4, precision="bf16")
    zs = zs.to(w.device)
    kw = _model_kwargs(w, batch)
    for method in METHODS:
        a = w.model.sample_rk(zs, method, 4, use_graph=True, **kw)      # captured
        b = w.model.sample_rk(zs, method, 4, use_graph=True, **kw)      # replayed
        c = w.model.sample_rk(zs, method, 4, use_graph=False, **kw)
        assert torch.isfinite(a).all() and not torch.equal(a, zs)
        assert torch.equal(a, b) and torch.equal(a, c), method
    # a second shape (and another step count) in between does not disturb the first one's cached graph
    first = w.model.sample_rk(zs, "rk4", 4, use_graph=True, **kw)
    from mdgen_amd.synthetic import synth_batch
    batch2 = synth_batch(1, 8, 4, 0, w.device, seed=7)
    kw2 = _model_kwargs(w, batch2)
    zs2 = torch.randn(1, 8, 4, w.latent_dim, generator=torch.Generator().manual_seed(3)).to(w.device)
    other = w.model.sample_rk(zs2, "rk4", 4, use_graph=True, **kw2)
    more = w.model.sample_rk(zs, "rk4", 5, use_graph=True, **kw)
    again = w.model.sample_rk(zs, "rk4", 4, use_graph=True, **kw)
    assert torch.equal(first, again) and not torch.equal(first, more)
    assert torch.equal(other, w.model.sample_rk(zs2, "rk4", 4, use_graph=False, **kw2))


# ---- 10: batch independence ---------------------------------------------------------------------------------------------------
def test_rk4_batch_is_independent_solves():
    """Every sample sees the same time grid: a B = 3 call is three B = 1 solves (contrast test_dopri5_batch_shares_one_step_size).
    The two sides differ only in which kernel forms a launch size picks; Euler's value for the same comparison is printed
    beside it, and if that already exceeds 1e-5 the gate is 4 x Euler's."""
    B, T, L_ = 3, 40, 4
    w, _, _, batch, zs = _wrapper(B, T, L_, wseed=3, bseed=11, zseed=2)
    zs = zs.to(w.device)
    zs[1] *= 0.5
    zs[2] *= 2.0
    kw = _model_kwargs(w, batch)

    def singles(fn):
        out = []
        for b in range(B):
            kb = _model_kwargs(w, {k: v[b:b + 1] for k, v in batch.items()})
            out.append(fn(zs[b:b + 1].contiguous(), kb))
        return torch.cat(out, 0)

    rk = lambda z, k_: w.model.sample_rk(z, "rk4", 6, **k_)
    eu = lambda z, k_: w.model.sample_euler(z, 24, **k_)
    e_rk = rel_l2(rk(zs, kw), singles(rk))
    e_eu = rel_l2(eu(zs, kw), singles(eu))
    gate = 1e-5 if e_eu <= 1e-5 else 4 * e_eu
    print(f"B = 3 call against three B = 1 calls: rk4 S=6 rel-L2 {e_rk:.2e}; Euler S=24 {e_eu:.2e}; gate {gate:.2e}")
    assert e_rk <= gate


# ---- 11: CLI ------------------------------------------------------------------------------------------------------------------
def test_sim_inference_cli_rk4_matches_python_api(tmp_path):
    import pandas as pd
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.geometry import restype_order, samples_to_atom14
    from mdgen_amd.rigid_utils import Rotation
    from mdgen_amd.synthetic import synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper
    from mdgen_amd import sim_inference as cli
    dev = _cuda()
    T, Rn, S = 24, 2, 4
    names = {"FLRH": "FLRH", "AWKD": "AWKD"}
    gen = torch.Generator().manual_seed(5)
    data = tmp_path / "data"
    data.mkdir()
    for n, sq in names.items():
        q = torch.randn(1, 4, 4, generator=gen)
        Rm = Rotation(quats=(q / q.norm(dim=-1, keepdim=True)).to(dev)).get_rot_mats()
        tr_ = torch.cumsum(2.2 * torch.randn(1, 4, 3, generator=gen), 1).to(dev)
        ang = 6.2831853 * torch.rand(1, 4, 7, generator=gen)
        lat = torch.zeros(1, 1, 4, 21, device=dev)
        lat[..., 0] = 1.0
        lat[..., 7:21] = torch.stack([ang.sin(), ang.cos()], -1).reshape(1, 1, 4, 14).to(dev)
        a14 = samples_to_atom14(lat, Rm, tr_, torch.tensor([[restype_order[c] for c in sq]], device=dev), tps=False)[0]
        np.save(data / f"{n}.npy", a14.cpu().numpy().repeat(3, 0).astype(np.float16))
    split = tmp_path / "split.csv"
    pd.DataFrame({"name": list(names), "seqres": list(names.values())}).to_csv(split, index=False)
    out = tmp_path / "out"
    base = ["--synthetic", "--data_dir", str(data), "--split", str(split), "--out_dir", str(out), "--num_frames", str(T),
            "--num_rollouts", str(Rn), "--npy"]
    torch.manual_seed(1234)
    res = cli.main(base + ["--sampling_method", "rk4", "--num_steps", str(S)])
    assert res["frames"] == len(names) * Rn * T
    # the same through the Python API, same seed: one inference(sampling_method="rk4") per block
    cfg = ModelConfig.forward_sim(num_frames=T)
    w = NewMDGenWrapper(cfg, device=dev)
    w.model.load_state_dict(synth_state_dict(cfg, 0))
    torch.manual_seed(1234)
    for n in names:
        batch = cli.make_group_batch([n], {n: np.load(data / f"{n}.npy")}, names, dev)
        blocks = []
        for _ in range(Rn):
            a14, batch = cli.rollout(w, batch, T, S, sampling_method="rk4")
            blocks.append(a14)
        api = torch.cat(blocks, 1)[0].cpu().numpy()
        got = np.load(out / f"{n}.npy")
        assert np.isfinite(got).all() and np.array_equal(got, api), n
