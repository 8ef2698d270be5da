"""The SDE sampler's in-kernel noise on the GPU (csrc/philox.h in csrc/k_sde.hip; mdgen_sample_sde_rng, mdgen_rollout_sde,
mdgen_upsample_sde): the generated noise against tests/philox_ref.py, the generator instantiation of the state kernels against the
buffer-reading one bit for bit -- alone and over whole solves --, graph replay on new seed words, the fused drivers against their
call-by-call routes, batch independence, the memory the path saves and the command line.  The helpers are tests/test_rk_gpu.py's,
tests/test_rk_drivers_gpu.py's and tests/test_upsampling_gpu.py's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import philox_ref as P
import test_rk_gpu as K
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEED = (0x5eed1e55 << 32) | 0x0badc0de      # a non-zero high word
FACTOR = 32.0


def _words(dev, seed=SEED, sample_base=0, block_base=0):
    from mdgen_amd import _lib as L
    return L.rng_words(seed, sample_base, block_base).to(dev)


def _opts(method, last, n=6):
    from mdgen_amd import _lib as L
    return L.sde_opts(method, "GVP", "sigma", 1.0, last, 0.04, n, 0.0)


# ---- 1: the generated noise against the numpy restatement ---------------------------------------------------------------------------
# (1, 1, 1): one element; (2, 3, 5): 315 elements a sample -- a 16-byte access straddles two samples, and 630 % 4 == 2 leaves a tail;
# (3, 40, 4): many 16-byte accesses per sample; (2, 6200, 4): the size at which the embedding takes its 128-token form
NOISE_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 40, 4), (2, 6200, 4)]


@pytest.mark.parametrize("shape", NOISE_SHAPES)
def test_generated_noise_vs_philox_ref(shape):
    """Gate: 32 x the largest error that the same formula, evaluated by torch in fp32 on the CPU on the same words, shows against
    fp64 (the words and both uniforms are exact: only sqrt, log, cos and two products round)."""
    from mdgen_amd import _lib as L
    dev = K._cuda()
    B, T, L_ = shape
    D, step, block, sample_base, block_base = 21, 7, 2, 5, 3
    rng = _words(dev, SEED, sample_base, block_base)
    got = L.sde_noise(B, T, L_, D, rng, step, block).cpu().double()
    ref, w = P.noise((B, T, L_, D), SEED, step, block=block_base + block, sample_base=sample_base)
    u1, u2 = (torch.from_numpy(u).float() for u in P.uniforms(w))
    cpu32 = torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(torch.tensor(6.2831855) * u2)
    ref = torch.from_numpy(ref)
    floor = float((cpu32.double() - ref).abs().max())
    err = float((got - ref).abs().max())
    print(f"{shape} x {D}: generated noise against fp64 {err:.3e}; torch fp32 on the CPU {floor:.3e} (gate x{FACTOR:.0f})")
    assert torch.isfinite(got).all() and float(got.abs().max()) <= 5.77
    assert err <= FACTOR * floor, (err, floor)


# ---- 2: the generator instantiation of k_sde_embed against the buffer-reading one --------------------------------------------------
X, NOISE, EM, PRED, HEUN_NOISE = 0, 1, 2, 3, 5
STAGES = [(X, "Euler", "Mean"), (NOISE, "Heun", "Tweedie"), (EM, "Euler", "Mean"), (PRED, "Heun", "Tweedie"), (HEUN_NOISE, "Heun", "Tweedie")]


@pytest.mark.parametrize("tps", [False, True])          # D = 21, D = 28
@pytest.mark.parametrize("shape", [(3, 11, 4), (2, 6200, 4)])   # 32-token workgroups (5 of them); 128-token ones
def test_embed_generator_form_equals_buffer_form(shape, tps):
    """States 1, 2, 5 (storing, noise-reading) and 0, 3 (not storing, no noise): the generator form's x and h equal, bit for bit,
    the buffer form's on the hook's noise of the step the state draws (state 5: step + 1)."""
    from mdgen_amd import _lib as L
    dev = K._cuda()
    B, T, L_ = shape
    model, _ = K._embed_model(tps, True, L_)
    D = model.cfg.latent_dim
    N = B * T * L_
    gen = torch.Generator().manual_seed(17 * B + D)
    x0 = torch.randn(B, T, L_, D, generator=gen).to(dev)
    v = [(torch.randn(B, T, L_, D, generator=gen) * s).to(dev) for s in (3.0, 0.5)]
    ipa = torch.randn(B * L_, 384, generator=gen).to(dev)
    x_cond, xcm = (a.to(dev) for a in K._cond_pattern("frame0", B, T, L_, D, gen))
    step, block = 2, 4
    rng = _words(dev, SEED, 9, 1)
    sh = L.Shape(B, T, L_)
    for code, method, last in STAGES:
        o = _opts(method, last)
        xi = L.sde_noise(B, T, L_, D, rng, step + 1 if code == HEUN_NOISE else step, block)
        xa, xb = x0.clone(), x0.clone()
        ha, hb = (torch.full((N, 384), float("nan"), device=dev) for _ in range(2))
        with torch.cuda.device(dev):
            L.check(L.lib.mdgen_debug_sde_stage(model._ctx, C.byref(sh), C.byref(o), code, step, L.ptr(xa), L.ptr(v[0]), L.ptr(v[1]),
                                                L.ptr(xi), L.ptr(x_cond), L.ptr(xcm), L.ptr(ipa), L.ptr(ha), L.stream_ptr()))
            L.check(L.lib.mdgen_debug_sde_stage_rng(model._ctx, C.byref(sh), C.byref(o), code, step, block, L.ptr(xb), L.ptr(v[0]),
                                                    L.ptr(v[1]), L.ptr(rng, torch.int64), L.ptr(x_cond), L.ptr(xcm), L.ptr(ipa), L.ptr(hb),
                                                    L.stream_ptr()))
        tag = (shape, D, code)
        assert torch.isfinite(hb).all(), tag
        assert torch.equal(xa, xb) and torch.equal(ha, hb), tag
        assert torch.equal(xb, x0) == (code in (X, PRED)), tag      # the noise-reading states store, and moved


# ---- 3: whole solves: the generator path equals the buffer path on the hook's noise -----------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup():
    return K._wrapper(2, 8, 5)


def _hook_noise(S, zs, rng, block=0):
    from mdgen_amd import _lib as L
    return torch.stack([L.sde_noise(*zs.shape, rng, i, block) for i in range(S)])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("method,last", [("Euler", "Mean"), ("Euler", None), ("Heun", "Tweedie"), ("Heun", None)])
def test_sample_sde_rng_equals_buffer_path_bit_for_bit(method, last, precision):
    w, _, _, batch, zs = _setup()
    w.model.set_precision(precision)
    dev = w.device
    zs = zs.to(dev)
    kw = K._model_kwargs(w, batch)
    o = _opts(method, last, n=5)
    rng = _words(dev, SEED, 3, 6)
    noise = _hook_noise(4, zs, rng)
    ref = w.model.sample_sde(zs, o, noise=noise, use_graph=False, **kw)
    assert torch.isfinite(ref).all() and not torch.equal(ref, zs)
    for use_graph in (False, True, True):
        got = w.model.sample_sde(zs, o, rng=rng, use_graph=use_graph, **kw)
        assert torch.equal(got, ref), (method, last, precision, use_graph)
    assert torch.equal(w.model.sample_sde(zs, o, noise=noise, use_graph=True, **kw), ref)
    w.model.set_precision("fp32")


# ---- 4: graph replay reads the seed words at replay ---------------------------------------------------------------------------------
def test_graph_replay_draws_from_the_words_it_finds():
    w, _, _, batch, zs = K._wrapper(2, 12, 4, precision="bf16")
    dev = w.device
    zs = zs.to(dev)
    for method, kwargs in (("sde", {}), ("sde_heun", dict(sde=dict(last_step="Tweedie")))):
        run = lambda seed, g, **k: (w.inference(batch, zs=zs, sampling_method=method, num_steps=4, rng_seed=seed, use_graph=g,
                                                **kwargs, **k), w.last_samples.clone())[1]
        a = run(1, True)                        # captured
        n = w.model.graph_count()
        b = run(2, True)                        # replayed on new words in the same buffer
        c = run(1, True)
        d = run(1, True, rng_sample_base=1)
        assert w.model.graph_count() == n, method
        assert torch.isfinite(a).all() and torch.equal(a, c) and not torch.equal(a, b) and not torch.equal(a, d)
        assert torch.equal(b, run(2, False)) and torch.equal(a, run(1, False)) and torch.equal(d, run(1, False, rng_sample_base=1))
    from mdgen_amd._lib import MdgenError
    with pytest.raises(MdgenError):
        w.inference(batch, zs=zs, sampling_method="sde", num_steps=4, rng_seed=1, noise=torch.zeros((4,) + tuple(zs.shape), device=dev))
    with pytest.raises(MdgenError):
        w.inference(batch, zs=zs, sampling_method="rk4", num_steps=4, rng_seed=1)


# ---- 5: the fused drivers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("method,sde", [("sde", None), ("sde_heun", dict(last_step="Tweedie", diffusion_form="linear"))])
def test_fused_rollout_sde_equals_the_chain_of_inference_calls(method, sde, precision):
    """rollout(rng_seed=s) over three blocks = inference(rng_seed=s, rng_block_base=0, 1, 2) + atom14_to_cond per block, bit for bit;
    ONE library call."""
    import test_rk_drivers_gpu as Dr
    from mdgen_amd.sim_inference import rollout as py_rollout
    B, T, L_, R_, S = 2, 12, 4, 3, 3
    w, _, _, batch, zs = Dr._setup(B, T, L_, R_)
    w.model.set_precision(precision)
    extra = {"sde": sde} if sde else {}
    blocks, samples, cur = [], [], dict(batch)
    for k, z in enumerate(zs):
        a, cur = py_rollout(w, cur, T, S, zs=z, sampling_method=method, rng_seed=SEED, rng_sample_base=4, rng_block_base=10 + k, **extra)
        blocks.append(a)
        samples.append(w.last_samples.clone())
    want = (torch.cat(blocks, 1), torch.stack(samples), cur)
    assert not torch.equal(samples[0], samples[1])
    calls = []
    orig = w.model.rollout_sde
    w.model.rollout_sde = lambda *a, **k: (calls.append(k.get("use_graph")), orig(*a, **k))[1]
    try:
        for use_graph in (False, True, True):
            a, nxt = w.rollout(batch, T, R_, num_steps=S, zs=zs, sampling_method=method, sde=sde, rng_seed=SEED, rng_sample_base=4,
                               rng_block_base=10, use_graph=use_graph, return_next=True)
            Dr._assert_same_rollout((a, w.last_samples.clone(), nxt), want, (method, precision, use_graph))
    finally:
        del w.model.rollout_sde
        w.model.set_precision("fp32")
    assert calls == [False, True, True]


def test_fused_upsample_sde_is_the_sum_of_its_parts():
    """upsample(rng_seed=s) = prep_keyframes -> sample_sde(rng words) -> samples_to_atom14, bit for bit; replayed on new key frames."""
    from mdgen_amd.geometry import prep_keyframes, samples_to_atom14
    from test_upsampling_gpu import case_2_12_4, key_frames, make_wrapper, to_dev
    dev = K._cuda()
    B, T, L_, c, S, kbA, _, zs = case_2_12_4()
    kbB, _ = key_frames(B, T, L_, c, 177)
    w, _, _ = make_wrapper(T, c)
    z = zs.to(dev)
    sde = dict(last_step="Euler", last_step_size=0.1)
    from mdgen_amd.solver import sde_opts
    o = sde_opts("sde_heun", 3, sde, "GVP")

    def parts(kb):
        kb = to_dev(kb, dev)
        p = prep_keyframes(kb["rots"], kb["trans"], kb["torsions"], T, c)
        mask = kb["mask"].float()[:, None].expand(B, T, L_).contiguous()
        s = w.model.sample_sde(z, o, mask=mask, start_frames=(p["start_rot"], p["start_trans"]), x_cond=p["x_cond"],
                               x_cond_mask=p["x_cond_mask"], aatype=kb["seqres"], use_graph=False, rng=_words(dev, 21, 2, 5))
        return samples_to_atom14(s, p["start_rot"], p["start_trans"], kb["seqres"], False), s
    refs = {"A": parts(kbA), "B": parts(kbB)}
    assert torch.isfinite(refs["A"][0]).all() and not torch.equal(refs["A"][1], refs["B"][1])
    for tag, kb, use_graph in (("A", kbA, False), ("A", kbA, True), ("A", kbA, True), ("B", kbB, True), ("A", kbA, True)):
        a14, _ = w.upsample(to_dev(kb, dev), zs=z, num_steps=3, sampling_method="sde_heun", sde=sde, rng_seed=21, rng_sample_base=2,
                            rng_block_base=5, use_graph=use_graph)
        assert torch.equal(w.last_samples, refs[tag][1]) and torch.equal(a14, refs[tag][0]), (tag, use_graph)


def test_a_sample_draws_the_same_noise_in_any_batch():
    """A B = 3 call against three B = 1 calls at rng_sample_base 0, 1, 2: the noise bit for bit (through the hook), the samples at
    the gate of test_sde_batch_is_independent_solves -- the two sides differ only in which kernel forms a launch size picks;
    Euler's value for the same comparison is printed beside it, and if that already exceeds 1e-5 the gate is 4 x Euler's."""
    from mdgen_amd import _lib as L
    B, T, L_ = 3, 40, 4
    w, _, _, batch, zs = K._wrapper(B, T, L_, wseed=3, bseed=11, zseed=2)
    dev = w.device
    zs = zs.to(dev)
    D = zs.shape[-1]
    for step in (0, 5):
        full = L.sde_noise(B, T, L_, D, _words(dev, SEED), step)
        for b in range(B):
            assert torch.equal(full[b:b + 1], L.sde_noise(1, T, L_, D, _words(dev, SEED, sample_base=b), step)), (step, b)
    kw = K._model_kwargs(w, batch)
    o = _opts("Heun", "Mean", n=7)

    def singles(fn):
        out = []
        for b in range(B):
            kb = K._model_kwargs(w, {k: v[b:b + 1] for k, v in batch.items()})
            out.append(fn(zs[b:b + 1].contiguous(), b, kb))
        return torch.cat(out, 0)

    sde = lambda z, b, k_: w.model.sample_sde(z, o, rng=_words(dev, SEED, sample_base=b), **k_)
    eu = lambda z, b, k_: w.model.sample_euler(z, 13, **k_)
    full, one = sde(zs, 0, kw), singles(sde)
    e_sde, e_row0 = rel_l2(full, one), rel_l2(full[:1], one[:1])
    e_eu = rel_l2(eu(zs, 0, kw), singles(eu))
    gate = 1e-5 if e_eu <= 1e-5 else 4 * e_eu
    print(f"B = 3 call against three B = 1 calls at sample bases 0, 1, 2: sde_heun 6 steps + Mean rel-L2 {e_sde:.2e} (row 0: {e_row0:.2e}); "
          f"Euler S=13 {e_eu:.2e}; gate {gate:.2e}")
    assert torch.isfinite(full).all() and e_sde <= gate and e_row0 <= gate


# ---- 6: memory ----------------------------------------------------------------------------------------------------------------------
def test_generated_noise_needs_no_noise_buffer():
    """(1, 64, 4), 200 steps: the default call stages S x state floats of noise; the rng_seed call's peak allocation lies below the
    default call's by at least 0.9 of that."""
    B, T, L_, S = 1, 64, 4, 200
    w, _, _, batch, zs = K._wrapper(B, T, L_, precision="bf16")
    dev = w.device
    zs = zs.to(dev)
    call = lambda **k: w.inference(batch, zs=zs, sampling_method="sde", num_steps=S, use_graph=False, **k)[0]
    call(rng_seed=1)                                   # the workspace and the staging set of the shape exist from here on
    peaks = {}
    for name, k in (("rng_seed", dict(rng_seed=2)), ("default", {})):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = call(**k)
        torch.cuda.synchronize(dev)
        peaks[name] = torch.cuda.max_memory_allocated(dev)
        assert torch.isfinite(out).all()
    noise_bytes = S * zs.numel() * 4
    saved = peaks["default"] - peaks["rng_seed"]
    print(f"(1, 64, 4) x 200 steps: peak {peaks['default']} bytes by default, {peaks['rng_seed']} with rng_seed: {saved} saved "
          f"({saved / noise_bytes:.2f} x the noise of {noise_bytes} bytes)")
    assert saved >= 0.9 * noise_bytes


# ---- 7: the command line ------------------------------------------------------------------------------------------------------------
def test_sim_inference_cli_sde_seed(tmp_path):
    """--sde_seed 7 twice (the same torch seed for the blocks' initial noise): identical files; --sde_seed 8: different ones."""
    import pandas as pd
    from mdgen_amd.geometry import restype_order, samples_to_atom14
    from mdgen_amd.rigid_utils import Rotation
    from mdgen_amd import sim_inference as cli
    dev = K._cuda()
    T, Rn = 12, 2
    names = {"FLRH": "FLRH", "AKLG": "AKLG"}
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

    def run(tag, seed):
        out = tmp_path / tag
        torch.manual_seed(1234)
        res = cli.main(["--synthetic", "--data_dir", str(data), "--split", str(split), "--out_dir", str(out), "--num_frames", str(T),
                        "--num_rollouts", str(Rn), "--npy", "--sampling_method", "sde", "--num_steps", "4", "--sde_seed", str(seed)])
        assert res["frames"] == len(names) * Rn * T
        return {n: np.load(out / f"{n}.npy") for n in names}
    a, b, c = run("a", 7), run("b", 7), run("c", 8)
    for n in names:
        assert a[n].shape[0] == Rn * T and np.isfinite(a[n]).all()
        assert np.array_equal(a[n], b[n]), n
        assert not np.array_equal(a[n], c[n]), n
