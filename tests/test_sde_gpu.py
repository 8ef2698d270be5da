"""The SDE sampler on the GPU (mdgen_sample_sde: csrc/sde.inc + csrc/k_sde.hip) against tests/sde_ref.py -- the torch restatement
of the reference's Sampler.sample_sde, itself checked against the reference in tests/test_sde_cpu.py -- : the state-forming
embedding kernel alone, the whole solve against the CPU oracle's forward and against a host loop over the library's own forward,
the bf16 path, capture and noise behaviour, batch independence, a padded noise stride, the wrapper and the CLI.  The helpers are
tests/test_rk_gpu.py's; the gates are its formulas, restated here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sde_ref as R
import test_rk_gpu as K
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# the gate of the embedding h (tests/test_rk_gpu.py, tests/ipa_ref.py): (largest row error / rms row norm, rel-L2) against fp64, at 32 x
# what torch's own fp32 evaluation of the same expression shows, and at least 32 fp32 ulps
FACTOR, ULPS = 32.0, 32.0 * 2.0 ** -24
STAGE_SHAPES = [(1, 5, 3), (3, 11, 4), (5, 999, 10)]
N_POINTS, STEP = 6, 2
# every state the solver forms: (state code, method, last step)
STATES = [(R.X, "Euler", "Mean"), (R.NOISE, "Heun", "Tweedie"), (R.EM, "Euler", "Mean"), (R.PRED, "Heun", "Tweedie"),
          (R.HEUN, "Heun", "Tweedie"), (R.HEUN_NOISE, "Heun", "Tweedie"), (R.TWEEDIE, "Heun", "Tweedie"), (R.EULER, "Euler", "Euler"),
          (R.MEAN, "Euler", "Mean")]
STORING = {R.NOISE, R.EM, R.HEUN, R.HEUN_NOISE, R.TWEEDIE, R.EULER, R.MEAN}


def _opts(method, last, path="GVP", form="sigma", norm=1.0, h=0.04, n=N_POINTS, eps=0.0):
    from mdgen_amd import _lib as L
    return L.sde_opts(method, path, form, norm, last, h, n, eps), (method, path, form, norm, last, h, n, eps)


def _noise(S, shape, seed):
    return torch.randn((S,) + tuple(shape), generator=torch.Generator().manual_seed(seed))


# ---- 1: k_sde_embed alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abs_pos", [True, False])
@pytest.mark.parametrize("tps", [False, True])
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_sde_embed_kernel_states_bit_for_bit_and_h_vs_fp64(shape, tps, abs_pos):
    from mdgen_amd import _lib as L
    dev = K._cuda()
    B, T, L_ = shape
    model, sd = K._embed_model(tps, abs_pos, L_)
    D = model.cfg.latent_dim
    N = B * T * L_
    gen = torch.Generator().manual_seed(2000 * B + L_)
    x0 = torch.randn(B, T, L_, D, generator=gen)
    v = [torch.randn(B, T, L_, D, generator=gen) * s for s in (3.0, 0.5)]
    xi = torch.randn(B, T, L_, D, generator=gen)
    ipa = torch.randn(B * L_, 384, generator=gen)
    # the two-sided model takes the Linear path with the SBDM diffusion (sample_eps > 0), the other GVP with sigma
    path, form, eps = ("Linear", "SBDM", 1e-3) if tps else ("GVP", "sigma", 0.0)
    combos = [(True, "frame0"), (False, "tiles")] if N > 10000 else [(i, c) for i in (True, False) for c in ("frame0", "tiles")]
    sh = L.Shape(B, T, L_)
    v_dev, xi_dev = [a.to(dev) for a in v], xi.to(dev)
    worst = (0.0, 0.0)
    for with_ipa, kind in combos:
        x_cond, xcm = K._cond_pattern(kind, B, T, L_, D, gen)
        xc_dev, xcm_dev = x_cond.to(dev), xcm.to(dev)
        ipa_dev = ipa.to(dev) if with_ipa else None
        for code, method, last in STATES:
            o, args = _opts(method, last, path=path, form=form, eps=eps)
            p32 = R.make_plan(*args, torch.float32, from_library=True)
            p64 = R.make_plan(*args, torch.float64, from_library=True)
            x32 = R.state(code, p32, STEP, x0, v[0], v[1], xi)
            x64 = R.state(code, p64, STEP, x0.double(), v[0].double(), v[1].double(), xi.double())
            ref = K._embedding(sd, x64, x_cond, xcm, ipa if with_ipa else None, abs_pos, torch.float64, dev)
            floor = K._rows(K._embedding(sd, x32, x_cond, xcm, ipa if with_ipa else None, abs_pos, torch.float32).to(dev), ref)
            x_dev = x0.to(dev)
            h = torch.full((N, 384), float("nan"), device=dev)
            with torch.cuda.device(dev):
                L.check(L.lib.mdgen_debug_sde_stage(model._ctx, C.byref(sh), C.byref(o), code, STEP, L.ptr(x_dev), L.ptr(v_dev[0]),
                                                    L.ptr(v_dev[1]), L.ptr(xi_dev), L.ptr(xc_dev), L.ptr(xcm_dev), L.ptr(ipa_dev),
                                                    L.ptr(h), L.stream_ptr()))
            got = K._rows(h, ref)
            gate = tuple(max(FACTOR * f, ULPS) for f in floor)
            worst = max(worst, (got[0] / max(floor[0], 1e-30), got[1] / max(floor[1], 1e-30)))
            tag = (shape, tps, abs_pos, with_ipa, kind, code)
            assert torch.isfinite(h).all(), tag
            assert got[0] <= gate[0] and got[1] <= gate[1], (tag, got, gate)
            # the stored state is sde_ref's fp32 value on the plan's coefficient bits, bit for bit; the others exist only in the launch
            assert torch.equal(x_dev.cpu(), x32 if code in STORING else x0), tag
    print(f"{shape} D {D} pos {abs_pos}: worst h error / fp32 floor: row max x{worst[0]:.2f}, rel-L2 x{worst[1]:.2f} (gate x{FACTOR:.0f})")


# ---- 2: whole solve, fp32 mode ----------------------------------------------------------------------------------------------------
SOLVES = [("Euler", "Mean"), ("Heun", "Tweedie")]


@functools.lru_cache(maxsize=None)
def _setup():
    B, T, L_ = 2, 16, 4
    w, sd, cfg, batch, zs = K._wrapper(B, T, L_)
    return w, sd, cfg, batch, zs, _noise(4, zs.shape, 77)


def _inference(w, batch, zs, noise, method, last, n_steps=4, **kw):
    name = "sde" if method == "Euler" else "sde_heun"
    atom14, _ = w.inference(batch, zs=zs.to(w.device), sampling_method=name, num_steps=n_steps, noise=noise.to(w.device),
                            sde=dict(last_step=last), **kw)
    return atom14, w.last_samples.clone()


@pytest.mark.parametrize("method,last", SOLVES)
def test_sde_fp32_vs_oracle(method, last):
    """Gates of test_rk_fp32_vs_oracle: samples rel-L2 <= 1e-5, atom14 within 1e-3 A."""
    from oracle import mdgen_oracle as O
    w, sd, cfg, batch, zs, noise = _setup()
    obatch = {k: v.cpu() for k, v in batch.items()}
    c = O.cfg_dict(cfg)
    prep = O.prep_batch(obatch, c)
    B = zs.shape[0]
    atom14, samples = _inference(w, batch, zs, noise, method, last)
    p = R.make_plan(method, "GVP", "sigma", 1.0, last, 0.04, 5, 0.0, torch.float32, from_library=True)
    mk = prep["model_kwargs"]
    ref = R.solve(lambda t, y: O.forward(sd, c, y, torch.ones(B) * t, **mk), zs, noise, p, method, last)
    e = rel_l2(samples.cpu(), ref)
    d = float((atom14.cpu() - O.postprocess(ref, prep["rigids"], obatch["seqres"], c)[0]).abs().max())
    print(f"{method} / {last}, 5 points: samples rel-L2 {e:.2e}, atom14 max {d:.2e} A")
    assert e <= 1e-5 and d <= 1e-3


@pytest.mark.parametrize("method,last", SOLVES)
def test_sde_vs_host_loop_over_library_forward(method, last):
    """Gate of test_rk_vs_host_loop_over_library_forward: rel-L2 <= 1e-5."""
    from mdgen_amd import _lib as L
    w, _, _, batch, zs, noise = _setup()
    dev = w.device
    kw = K._model_kwargs(w, batch)
    B = zs.shape[0]
    o, args = _opts(method, last, n=5)
    x = w.model.sample_sde(zs.to(dev), o, noise=noise.to(dev), **kw)
    p = R.make_plan(*args, torch.float32, from_library=True)
    p = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in p.items()}
    p["t"] = [[t.to(dev) for t in st] for st in p["t"]]
    p["c"] = [[tuple(c.to(dev) for c in cs) for cs in st] for st in p["c"]]
    p["c_last"] = tuple(c.to(dev) for c in p["c_last"])
    ref = R.solve(lambda t, y: w.model.forward(y, torch.ones(B, device=dev) * t, **kw), zs.to(dev), noise.to(dev), p, method, last)
    e = rel_l2(x, ref)
    print(f"{method} / {last}, 5 points: rel-L2 against the host loop {e:.2e}")
    assert torch.isfinite(x).all() and e <= 1e-5


# ---- 3: bf16 path against fp32 mode -----------------------------------------------------------------------------------------------
def test_sde_bf16_vs_fp32_mode():
    """Gates of test_rk4_bf16_vs_fp32_mode: samples rel-L2 <= 1e-2, atom14 rms <= 0.02 A."""
    w, _, _, batch, zs = K._wrapper(2, 12, 4)
    noise = _noise(12, zs.shape, 78)
    a32, s32 = _inference(w, batch, zs, noise, "Euler", "Mean", n_steps=12)
    w.model.set_precision("bf16")
    a16, s16 = _inference(w, batch, zs, noise, "Euler", "Mean", n_steps=12)
    m = batch["mask"][:, None, :, None, None].bool()
    d = (a16 - a32).masked_select(m.expand_as(a16))
    e, rms = rel_l2(s16, s32), float(d.pow(2).mean().sqrt())
    print(f"sde 12 steps + Mean, bf16 against fp32 mode: samples rel-L2 {e:.2e}, atom14 rms {rms:.4f} A")
    assert torch.isfinite(a16).all() and torch.isfinite(s16).all()
    assert e <= 1e-2 and rms <= 0.02


# ---- 4: capture and noise ---------------------------------------------------------------------------------------------------------
def test_sde_graph_replay_and_noise():
    w, _, _, batch, zs = K._wrapper(2, 12, 4, precision="bf16")
    dev = w.device
    zs = zs.to(dev)
    kw = K._model_kwargs(w, batch)
    n1, n2 = _noise(4, zs.shape, 1).to(dev), _noise(4, zs.shape, 2).to(dev)
    for method, last in (("Euler", "Mean"), ("Heun", "Tweedie"), ("Heun", None), ("Euler", None)):
        o, _ = _opts(method, last, n=5)
        a = w.model.sample_sde(zs, o, noise=n1, use_graph=True, **kw)      # captured
        b = w.model.sample_sde(zs, o, noise=n1, use_graph=True, **kw)      # replayed
        c = w.model.sample_sde(zs, o, noise=n1, use_graph=False, **kw)
        assert torch.isfinite(a).all() and not torch.equal(a, zs)
        assert torch.equal(a, b) and torch.equal(a, c), (method, last)
        # the caller owns the noise: the same graph with new noise in the same buffer gives a new sample, the old noise the old one
        d = w.model.sample_sde(zs, o, noise=n2, use_graph=True, **kw)
        assert torch.isfinite(d).all() and not torch.equal(a, d), (method, last)
        assert torch.equal(d, w.model.sample_sde(zs, o, noise=n2, use_graph=False, **kw))
        assert torch.equal(a, w.model.sample_sde(zs, o, noise=n1, use_graph=True, **kw))
    # without noise the draw is the device generator's: the seed decides the sample
    o, _ = _opts("Euler", "Mean", n=5)
    torch.manual_seed(11)
    a = w.model.sample_sde(zs, o, **kw)
    torch.manual_seed(11)
    b = w.model.sample_sde(zs, o, **kw)
    c = w.model.sample_sde(zs, o, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_sde_without_diffusion_is_the_euler_sampler():
    """Zero noise, diffusion_norm = 0 and an Euler last step of size 1 - t1: the steps are x + v dt on t = 0, 1/5, .. 4/5, what
    sample_euler takes in 5 steps (grid values and dt agree to fp32 rounding) -- to the gate of the RK host-loop test, in fp32 mode."""
    w, _, _, batch, zs, _ = _setup()
    dev = w.device
    kw = K._model_kwargs(w, batch)
    o, _ = _opts("Euler", "Euler", form="constant", norm=0.0, h=0.2, n=5)
    x = w.model.sample_sde(zs.to(dev), o, noise=torch.zeros((4,) + tuple(zs.shape), device=dev), **kw)
    ref = w.model.sample_euler(zs.to(dev), 5, **kw)
    e = rel_l2(x, ref)
    print(f"sde with D = 0, zero noise, Euler last step against sample_euler(5 steps): rel-L2 {e:.2e}")
    assert e <= 1e-5


# ---- 5: batch independence --------------------------------------------------------------------------------------------------------
def test_sde_batch_is_independent_solves():
    """A B = 3 call is three B = 1 solves, each with its row of the noise.  The two sides differ only in which kernel forms a launch
    size picks (test_rk4_batch_is_independent_solves): Euler's value for the same comparison is printed beside it, and if that
    already exceeds 1e-5 the gate is 4 x Euler's."""
    B, T, L_ = 3, 40, 4
    w, _, _, batch, zs = K._wrapper(B, T, L_, wseed=3, bseed=11, zseed=2)
    zs = zs.to(w.device)
    noise = _noise(6, zs.shape, 5).to(w.device)
    kw = K._model_kwargs(w, batch)
    o, _ = _opts("Heun", "Mean", n=7)

    def singles(fn):
        out = []
        for b in range(B):
            kb = K._model_kwargs(w, {k: v[b:b + 1] for k, v in batch.items()})
            out.append(fn(zs[b:b + 1].contiguous(), noise[:, b:b + 1].contiguous(), kb))
        return torch.cat(out, 0)

    sde = lambda z, n, k_: w.model.sample_sde(z, o, noise=n, **k_)
    eu = lambda z, n, k_: w.model.sample_euler(z, 13, **k_)
    full = sde(zs, noise, kw)
    one = singles(sde)
    e_sde, e_row0 = rel_l2(full, one), rel_l2(full[:1], one[:1])
    e_eu = rel_l2(eu(zs, noise, kw), singles(eu))
    gate = 1e-5 if e_eu <= 1e-5 else 4 * e_eu
    print(f"B = 3 call against three B = 1 calls: sde_heun 6 steps + Mean rel-L2 {e_sde:.2e} (row 0: {e_row0:.2e}); Euler S=13 {e_eu:.2e}; gate {gate:.2e}")
    assert e_sde <= gate and e_row0 <= gate


# ---- 6: a padded noise stride, a state that does not end on 16 bytes --------------------------------------------------------------
def test_sde_padded_noise_stride_and_odd_state():
    from mdgen_amd import _lib as L
    B, T, L_ = 1, 5, 3       # 315 floats: 315 % 4 == 3
    w, _, _, batch, zs = K._wrapper(B, T, L_)
    dev = w.device
    zs = zs.to(dev)
    kw = K._model_kwargs(w, batch)
    noise = _noise(4, zs.shape, 9).to(dev)
    for method, last in (("Euler", "Mean"), ("Heun", None)):
        o, args = _opts(method, last, n=5)
        a = w.model.sample_sde(zs, o, noise=noise, **kw)                               # stride 316
        b = w.model.sample_sde(zs, o, noise=noise, noise_step_stride=332, **kw)
        c = w.model.sample_sde(zs, o, noise=noise, noise_step_stride=332, use_graph=False, **kw)
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), (method, last)
        p = R.make_plan(*args, torch.float32, from_library=True)
        ref = R.solve(lambda t, y: w.model.forward(y.to(dev), torch.ones(B, device=dev) * t.to(dev), **kw).cpu(), zs.cpu(), noise.cpu(), p,
                      method, last)
        e = rel_l2(a.cpu(), ref)
        print(f"(1, 5, 3) {method} / {last}: rel-L2 against the host loop {e:.2e}")
        assert e <= 1e-5
    for stride in (318, 312):   # not a multiple of 4; below one state
        with pytest.raises(L.MdgenError):
            w.model.sample_sde(zs, o, noise=noise, noise_step_stride=stride, **kw)
    # a workspace one byte short is refused with -7
    sh = L.Shape(B, T, L_)
    nbytes = C.c_size_t()
    L.check(L.lib.mdgen_sde_workspace_bytes(w.model._ctx, C.byref(sh), C.byref(o), C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    x = zs.clone()
    nbuf = torch.zeros(4, 316, device=dev)
    some = L.ptr(torch.zeros(B * T * L_ * 28, device=dev))   # (the size is judged before any pointer is followed)
    cond = L.Cond(mask=some, start_rot=some, start_trans=some, x_cond=some, x_cond_mask=some, aatype=some)
    with torch.cuda.device(dev):
        rc = L.lib.mdgen_sample_sde(w.model._ctx, C.byref(sh), C.byref(o), L.ptr(x), L.ptr(nbuf), 316, C.byref(cond), L.ptr(ws),
                                    nbytes.value - 1, 0, L.stream_ptr())
    assert rc == -7 and b"workspace too small" in L.lib.mdgen_last_error()
    assert torch.equal(x, zs)


# ---- 7: the wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_inference_sde_is_seeded_and_finite():
    B, T, L_ = 2, 12, 4
    w, _, _, batch, _ = K._wrapper(B, T, L_, precision="bf16")
    torch.manual_seed(21)
    a, aa = w.inference(batch, sampling_method="sde")          # 49 steps + Mean, the "sigma" diffusion
    sa = w.last_samples.clone()
    torch.manual_seed(21)
    b, _ = w.inference(batch, sampling_method="sde")
    c, _ = w.inference(batch, sampling_method="sde")
    assert a.shape == (B, T, L_, 14, 3) and aa.shape == (B, T, L_) and sa.shape == (B, T, L_, w.latent_dim)
    assert torch.isfinite(a).all() and torch.isfinite(sa).all()
    assert torch.equal(a, b) and not torch.equal(a, c)
    h, _ = w.inference(batch, sampling_method="sde_heun", num_steps=3, sde=dict(last_step="Tweedie", diffusion_form="linear"))
    assert torch.isfinite(h).all() and h.shape == a.shape


# ---- 7a: rollout() and upsample() take the two names as host loops ---------------------------------------------------------------
def test_rollout_sde_is_the_chain_of_inference_calls():
    """rollout(sampling_method="sde") is the per-block loop of sim_inference.rollout: the same draws from the same seed, the same bits."""
    import test_rk_drivers_gpu as Dr
    B, T, L_, R_ = 2, 12, 4, 2
    w, _, _, batch, zs = Dr._setup(B, T, L_, R_)
    for method, sde in (("sde", None), ("sde_heun", dict(last_step="Tweedie", diffusion_form="linear"))):
        from mdgen_amd.sim_inference import rollout as py_rollout
        torch.manual_seed(5)
        blocks, samples, cur = [], [], dict(batch)
        for z in zs:
            a, cur = py_rollout(w, cur, T, 3, zs=z, sampling_method=method, **({"sde": sde} if sde else {}))
            blocks.append(a)
            samples.append(w.last_samples.clone())
        torch.manual_seed(5)
        a, nxt = w.rollout(batch, T, R_, num_steps=3, zs=zs, sampling_method=method, sde=sde, return_next=True)
        Dr._assert_same_rollout((a, w.last_samples.clone(), nxt), (torch.cat(blocks, 1), torch.stack(samples), cur), method)
        assert a.shape == (B, R_ * T, L_, 14, 3)


def test_upsample_sde_route():
    """upsample(sampling_method="sde") = prep_keyframes -> sample_sde -> samples_to_atom14 equals inference(window batch,
    sampling_method="sde") bitwise under the same seed (the two preparations agree bit for bit, tests/test_upsampling_gpu.py)."""
    import test_upsampling_gpu as U
    from mdgen_amd._lib import MdgenError
    dev = K._cuda()
    B, T, L_, c = 1, 8, 4, 4
    kb, wb = U.key_frames(B, T, L_, c, 61)
    w, _, _ = U.make_wrapper(T, c)
    z = torch.randn(B, T, L_, 21, generator=torch.Generator().manual_seed(62)).to(dev)
    sde = dict(last_step="Euler", last_step_size=0.1)
    torch.manual_seed(8)
    a_up, _ = w.upsample(U.to_dev(kb, dev), zs=z, sampling_method="sde_heun", num_steps=3, sde=sde)
    s_up = w.last_samples.clone()
    torch.manual_seed(8)
    a_inf, _ = w.inference(U.to_dev(wb, dev), zs=z, sampling_method="sde_heun", num_steps=3, sde=sde)
    assert torch.isfinite(a_up).all() and a_up.shape == (B, T, L_, 14, 3)
    assert torch.equal(s_up, w.last_samples) and torch.equal(a_up, a_inf)
    with pytest.raises(MdgenError):   # the options go with the SDE methods only
        w.upsample(U.to_dev(kb, dev), zs=z, sampling_method="rk4", sde=sde)


# ---- 8: CLI -----------------------------------------------------------------------------------------------------------------------
def test_sim_inference_cli_sde(tmp_path):
    import pandas as pd
    from mdgen_amd.geometry import restype_order, samples_to_atom14
    from mdgen_amd.rigid_utils import Rotation
    from mdgen_amd import sim_inference as cli
    dev = K._cuda()
    T, Rn = 24, 2
    names = {"FLRH": "FLRH"}
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
    torch.manual_seed(1234)
    res = cli.main(["--synthetic", "--data_dir", str(data), "--split", str(split), "--out_dir", str(out), "--num_frames", str(T),
                    "--num_rollouts", str(Rn), "--npy", "--sampling_method", "sde", "--num_steps", "4"])
    assert res["frames"] == len(names) * Rn * T
    got = np.load(out / "FLRH.npy")
    assert got.shape[0] == Rn * T and np.isfinite(got).all()
