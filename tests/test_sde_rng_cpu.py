"""The SDE sampler's generated noise without a GPU: Philox4x32-10 (csrc/philox.h through mdgen_debug_philox) against Random123's known
answers and against tests/philox_ref.py, the statistics of the stream the header describes, and the surface of the new entry points
(mdgen_sample_sde_rng, mdgen_rollout_sde, mdgen_upsample_sde): header / exports / binding, refusals before any device call,
resolve_solver and the command lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mdgen_sample_sde_rng", "mdgen_rollout_sde", "mdgen_upsample_sde", "mdgen_debug_sde_noise", "mdgen_debug_sde_stage_rng",
       "mdgen_debug_philox", "mdgen_debug_graph_count"]

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ---- 1: the generator ---------------------------------------------------------------------------------------------------------------
def test_philox_known_answers_and_reference():
    from mdgen_amd import _lib as L
    from mdgen_amd import philox as H
    for ctr, key, want in KNOWN:
        assert tuple(int(v) for v in L.philox(ctr, key)) == want, ctr
        assert tuple(int(v) for v in P.philox(np.array(ctr, dtype=np.uint32), key)) == want, ctr
        assert tuple(int(v) for v in H.philox4x32_10(*ctr, *key)) == want, ctr
    g = np.random.default_rng(5)
    ctrs = g.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64).astype(np.uint32)
    keys = g.integers(0, 2 ** 32, size=(300, 2), dtype=np.uint64).astype(np.uint32)
    for c, k in zip(ctrs, keys):
        assert np.array_equal(L.philox(c, k), P.philox(c, k)), (c, k)
    assert L.lib.mdgen_debug_philox(None, None, None) == -1


def test_package_restatement_is_the_reference_stream():
    """mdgen_amd.philox.sde_noise (what Sampler.sample_sde's host loop integrates) against philox_ref: the same words, so the fp32
    deviates agree with the fp64 ones to the rounding of sqrt / log / cos on values below 5.77."""
    from mdgen_amd import philox as H
    shape, seed = (2, 3, 5, 21), (0x9abcdef1 << 32) | 1234
    z64, w = P.noise(shape, seed, step=3, block=2 + 7, sample_base=2 ** 32 - 1)     # the sample word wraps
    z32 = H.sde_noise(shape, seed, 3, block_base=2, sample_base=2 ** 32 - 1, block=7)
    assert z32.dtype == np.float32 and z32.shape == shape
    assert np.abs(z32 - z64).max() <= 32 * 2.0 ** -24 * 5.77
    assert np.array_equal(w[1, 0, 0, 0, :2], P.philox(np.array([0, 0, 3, 9], dtype=np.uint32), P.key_of(seed))[:2])
    u1, u2 = P.uniforms(w)
    assert u1.min() >= 2.0 ** -24 and u1.max() < 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    with pytest.raises(ValueError):
        H.sde_noise((1, 2 ** 16, 2 ** 16, 21), 1, 0)


def test_stream_statistics():
    """n = 2^18 deviates of the stream (a (4, 64, 16, 64) state): first moments within 5 standard errors of N(0, 1)'s, and no
    correlation beyond 5 / sqrt(n) with the stream one element, sample, step, block or seed away."""
    seed, n = 1234, 2 ** 18
    T, L_, D = 64, 16, 64
    shape = (4, T, L_, D)
    z = P.noise(shape, seed, step=0)[0]
    x = z.reshape(-1)
    assert x.size == n
    mean, var = x.mean(), x.var()
    m4 = ((x - mean) ** 4).mean() / var ** 2
    s = (abs(mean) * np.sqrt(n), abs(var - 1) / np.sqrt(2 / n), abs(m4 - 3) / np.sqrt(96 / n))
    print(f"n = 2^18 at seed {seed}: |mean| sqrt(n) {s[0]:.2f}, |var - 1| / sqrt(2 / n) {s[1]:.2f}, |m4 - 3| / sqrt(96 / n) {s[2]:.2f}")
    assert max(s) <= 5, s
    assert np.abs(x).max() <= 5.77

    def corr(a, b):
        a, b = a.reshape(-1), b.reshape(-1)
        return abs(np.corrcoef(a, b)[0, 1])
    flat = z.reshape(4, -1)
    others = {"element + 1": (flat[:, :-1], flat[:, 1:]),
              "sample + 1": (z, P.noise(shape, seed, step=0, sample_base=1)[0]),
              "step + 1": (z, P.noise(shape, seed, step=1)[0]),
              "block + 1": (z, P.noise(shape, seed, step=0, block=1)[0]),
              "seed + 1": (z, P.noise(shape, seed + 1, step=0)[0])}
    # (sample + 1 shares three of four samples with z, shifted by one: the comparison is sample b against sample b + 1)
    for name, (a, b) in others.items():
        c = corr(a, b) * np.sqrt(n)
        print(f"  correlation with {name}: {c:.2f} / sqrt(n)")
        assert c <= 5, (name, c)


# ---- 2: the surface -----------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree():
    from mdgen_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    declared = set(re.findall(r"\b(mdgen_\w+)\s*\(", hdr))
    for n in NEW:
        assert n in L.EXPORTS and n in declared and hasattr(L.lib, n) and getattr(L.lib, n).argtypes is not None, n
    assert "#define MDGEN_ABI_VERSION 8" in hdr and L.lib.mdgen_abi_version() == 8
    # the header states the stream: the constants and the counter layout
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "sample_base + b", "block_base + k", "(t L + l) D + d"):
        assert word in hdr, word
    w = L.rng_words((5 << 32) | 7, 2 ** 32 + 3, 9)
    assert w.tolist() == [(5 << 32) | 7, 3, 9, 0] and L.rng_words(2 ** 64 - 1).tolist() == [-1, 0, 0, 0]


def _raw_opts(**kw):
    from mdgen_amd import _lib as L
    d = dict(method=1, path=1, diffusion_form=2, last_step=1, n_points=6, diffusion_norm=1.0, last_step_size=0.04, sample_eps=0.0)
    d.update(kw)
    return L.SdeOpts(**d)


BAD_OPTS = [dict(method=0), dict(path=2), dict(diffusion_form=6), dict(last_step=4), dict(n_points=1), dict(last_step_size=1.0),
            dict(sample_eps=1.0), dict(diffusion_form=1, sample_eps=0.0), dict(path=0, method=2, last_step=0)]


def test_library_refusals_come_before_any_device_call():
    """No context, no device, pointers that must not be followed: every refusal below is decided on the host."""
    from mdgen_amd import _lib as L
    lib = L.lib
    sh = L.Shape(1, 8, 4)
    fake = C.c_void_p(4096)
    cond = L.Cond(mask=fake, start_rot=fake, start_trans=fake, x_cond=fake, x_cond_mask=fake, aatype=fake)
    tb = L.ResidueTables(*([fake] * 8))
    ok = _raw_opts()

    def ref(o):
        return C.byref(o) if o is not None else None

    def sample(o=ok, x=fake, rng=fake, cd=cond, shape=sh):
        return lib.mdgen_sample_sde_rng(None, C.byref(shape), ref(o), x, rng, ref(cd), fake, 1 << 30, 0, None)

    def rollout(o=ok, rng=fake, n_blocks=2, zs=fake, stride=672, tables=tb, ctors=fake, shape=sh):
        return lib.mdgen_rollout_sde(None, C.byref(shape), ref(o), rng, n_blocks, zs, stride, fake, fake, fake, ctors, fake, fake, fake,
                                     ref(tables), fake, fake, 1 << 30, 0, None)

    def upsample(o=ok, rng=fake, interval=2, zs=fake, tables=tb, keys=fake):
        return lib.mdgen_upsample_sde(None, C.byref(sh), ref(o), rng, interval, zs, fake, keys, fake, fake, fake, fake, fake, fake, fake,
                                      ref(tables), fake, fake, 1 << 30, 0, None)

    for kw in BAD_OPTS:
        o = _raw_opts(**kw)
        assert sample(o) == -2 and rollout(o) == -2 and upsample(o) == -2, (kw, lib.mdgen_last_error())
    # null arguments
    assert sample(o=None) == -1 and sample(x=None) == -1 and sample(rng=None) == -1 and sample(cd=None) == -1
    for missing in ("mask", "start_rot", "start_trans", "x_cond", "x_cond_mask", "aatype"):
        cd = L.Cond(mask=fake, start_rot=fake, start_trans=fake, x_cond=fake, x_cond_mask=fake, aatype=fake)
        setattr(cd, missing, None)
        assert sample(cd=cd) == -1, missing
    assert rollout(o=None) == -1 and rollout(rng=None) == -1 and rollout(zs=None) == -1 and rollout(tables=None) == -1
    assert rollout(ctors=None) == -1
    assert upsample(o=None) == -1 and upsample(rng=None) == -1 and upsample(zs=None) == -1 and upsample(tables=None) == -1
    assert upsample(keys=None) == -1
    part = L.ResidueTables(*([fake] * 4 + [None] * 4))
    assert rollout(tables=part) == -1 and b"residue table" in lib.mdgen_last_error()
    # counts, alignment, stride (a block of (1, 8, 4) x 21 = 672 floats)
    assert rollout(n_blocks=0) == -2 and upsample(interval=0) == -2
    assert sample(x=C.c_void_p(4100)) == -7 and sample(rng=C.c_void_p(4100)) == -7 and b"8-byte" in lib.mdgen_last_error()
    assert rollout(zs=C.c_void_p(4100)) == -7 and upsample(zs=C.c_void_p(4104)) == -7
    assert rollout(stride=674) == -7 and b"multiple of 4" in lib.mdgen_last_error()
    assert rollout(stride=668) == -7 and b"below one block" in lib.mdgen_last_error()
    # the element counter has 32 bits: T L D >= 2^32 is refused whatever else the shape would run into
    big = L.Shape(1, 16384, 16384)
    assert sample(shape=big) == -2 and b"32-bit element counter" in lib.mdgen_last_error()
    assert lib.mdgen_debug_sde_noise(C.byref(big), 21, fake, 0, 0, fake, None) == -2
    # with everything in order the call gets as far as the context (null here): still no device call
    assert sample() == -1 and rollout() == -1 and upsample() == -1
    # the hooks
    assert lib.mdgen_debug_sde_noise(None, 21, fake, 0, 0, fake, None) == -1
    assert lib.mdgen_debug_sde_noise(C.byref(sh), 21, None, 0, 0, fake, None) == -1
    assert lib.mdgen_debug_sde_noise(C.byref(sh), 21, fake, 0, 0, C.c_void_p(4100), None) == -7
    assert lib.mdgen_debug_sde_stage_rng(None, C.byref(sh), C.byref(ok), 1, 0, 0, fake, None, None, None, fake, fake, None, fake, None) == -1


def test_resolve_solver_judges_the_seed():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.solver import resolve_solver
    c = resolve_solver("euler", "sde", 4, rng_seed=7)
    assert c.kind == "sde" and c.rng_seed == 7 and c.steps == 4
    assert resolve_solver("euler", "sde_heun", 4, rng_seed=0).rng_seed == 0          # seed 0 is a seed
    assert resolve_solver("euler", "sde", 4).rng_seed is None
    for method in (None, "euler", "rk4", "midpoint", "dopri5"):
        with pytest.raises(MdgenError, match="rng_seed"):
            resolve_solver("euler", method, None if method == "dopri5" else 4, rng_seed=7)
    with pytest.raises(MdgenError, match="one or the other"):
        resolve_solver("euler", "sde", 4, noise=object(), rng_seed=7)
    with pytest.raises(MdgenError, match="rng_seed"):
        resolve_solver("euler", "sde", 4, rng_sample_base=3)                         # an index of a stream nobody asked for
    with pytest.raises(MdgenError):
        resolve_solver("euler", "sde", 4, rng_seed=7, rng_sample_base=-1)


def test_sampler_function_refuses_seed_with_noise_and_draws_the_stream():
    """Sampler.sample_sde's function with a generic callable: `rng_seed` integrates mdgen_amd.philox's noise -- the result equals
    the same call handed that noise as `noise` -- and goes with no `noise`."""
    import torch
    from mdgen_amd import _lib as L
    from mdgen_amd import philox as H
    from mdgen_amd.transport import Sampler, create_transport
    fn = Sampler(create_transport(None, "GVP", "velocity")).sample_sde(diffusion_form="sigma", num_steps=5)
    f = lambda x, t: -x * t.view(-1, 1, 1, 1)
    x0 = torch.randn(2, 3, 4, 21, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    a = fn(x0, f, rng_seed=11, rng_sample_base=5, rng_block_base=2)
    noise = torch.stack([torch.from_numpy(H.sde_noise(x0.shape, 11, i, 2, 5)) for i in range(4)]).double()
    assert torch.equal(a, fn(x0, f, noise=noise)) and not torch.equal(a, fn(x0, f, rng_seed=12, rng_sample_base=5, rng_block_base=2))
    with pytest.raises(L.MdgenError):
        fn(x0, f, noise=noise, rng_seed=11)


@pytest.mark.parametrize("cli", ["sim_inference", "tps_inference", "upsampling_inference"])
def test_cli_accepts_the_seed_with_sde_and_exits_without(cli, tmp_path):
    import importlib
    from mdgen_amd.solver import sde_kwargs, solver_kwargs
    mod = importlib.import_module("mdgen_amd." + cli)
    base = ["--data_dir", str(tmp_path), "--synthetic"]
    entry = mod.parse_args if hasattr(mod, "parse_args") else mod.main
    for extra in (["--sde_seed", "7"], ["--sampling_method", "euler", "--sde_seed", "7"], ["--sampling_method", "rk4", "--sde_seed", "7"],
                  ["--sampling_method", "dopri5", "--sde_seed", "7"], ["--sampling_method", "sde", "--sde_seed", "seven"]):
        with pytest.raises(SystemExit):
            entry(base + extra)
    a = mod.build_parser().parse_args(base + ["--sampling_method", "sde", "--sde_seed", "7", "--num_steps", "4"])
    assert a.sde_seed == 7 and sde_kwargs(a) == {"sde": {}, "rng_seed": 7}
    assert solver_kwargs(a) == dict(num_steps=4, sampling_method="sde", sde={}, rng_seed=7)
    a = mod.build_parser().parse_args(base + ["--sampling_method", "sde_heun", "--sde_seed", "0", "--last_step", "Tweedie"])
    assert sde_kwargs(a) == {"sde": dict(last_step="Tweedie"), "rng_seed": 0}
    assert mod.build_parser().parse_args(base + ["--sampling_method", "sde"]).sde_seed is None
