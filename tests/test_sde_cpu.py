"""Host-only checks of the SDE sampler (csrc/sde.inc, mdgen_amd/transport.py): tests/sde_ref.py against the reference's own
Sampler.sample_sde (tests/golden/sde_toy.npz, written by scripts/gen_golden_sde.py), the library's plan bit for bit, the refusals,
the generic-callable path of Sampler.sample_sde, the dispatch plan of one step, and the exported names."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sde_ref as R
from conftest import rel_l2

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.golden_cases()
ALL_FORMS = ("constant",) + R.FORMS


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sde_toy.npz"))
    return {k: g[k] for k in g.files}


def _f(t, x):
    return R.toy(x, t)


# ---- 1: sde_ref in fp64 against the reference ------------------------------------------------------------------------------------
def test_sde_ref_fp64_matches_the_reference_on_every_golden_row(gold):
    """sde_ref differs from the reference only by fp64 rounding (it multiplies by iV where the reference divides, and evaluates the
    model once per state): with at most 11 evaluations of smooth maps, 1e-10 separates that from a restated formula."""
    assert len(CASES) == 80 + 48 and len({R.golden_key(*c) for c in CASES}) == len(CASES)
    init, noise = torch.from_numpy(gold["init"]), torch.from_numpy(gold["noise"])
    n, h, norm = int(gold["n_points"]), float(gold["last_step_size"]), float(gold["diffusion_norm"])
    assert init.shape == (2, 3, 4, 21) and n == 6 and noise.shape == (5, 2, 3, 4, 21)
    worst = 0.0
    for path, form, method, last, eps in CASES:
        p = R.make_plan(method, path, form, norm, last, h, n, eps, torch.float64)
        got = R.solve(_f, init, noise, p, method, last)
        e = rel_l2(got, torch.from_numpy(gold[R.golden_key(path, form, method, last, eps)]))
        worst = max(worst, e)
        assert e <= 1e-10, (path, form, method, last, eps, e)
    print(f"sde_ref fp64 against the reference's sample_sde, {len(CASES)} combinations: worst rel-L2 {worst:.2e}")


# ---- 2: the library's plan --------------------------------------------------------------------------------------------------------
def _ulp_distance(a, b):
    """|a - b| in units of b's fp32 ulp (b: the fp64 value)."""
    b32 = np.float32(b)
    ulp = np.spacing(np.abs(b32)) if b32 != 0 else np.float32(2.0 ** -149)
    return abs(float(a) - float(b)) / float(ulp)


@pytest.mark.parametrize("eps", [1e-3, 0.0])
@pytest.mark.parametrize("path", R.PATHS)
@pytest.mark.parametrize("method", R.METHODS)
def test_plan_rows_and_coefficients(method, path, eps):
    from mdgen_amd import _lib as L
    stages = R.METHODS.index(method) + 1
    differ = 0
    for form in ALL_FORMS:
        for last in R.LAST_STEPS:
            for n, h, norm in ((6, 0.04, 1.0), (2, 0.25, 0.7), (50, 0.04, 1.3)):
                if eps == 0.0 and (form == "SBDM" or (path == "Linear" and method == "Heun" and last is None)):
                    continue   # refused: test_library_refusals
                lp = L.sde_plan(L.sde_opts(method, path, form, norm, last, h, n, eps))
                S = n - 1
                t0, t1, hh = R.interval(form, last, h, eps)
                tg = R.grid(t0, t1, n, np.float32)
                dt = tg[1] - tg[0]
                rows = lp["rows"].view(np.float32)
                assert lp["row_of"].shape == (S, stages)
                assert lp["dt"].view(np.uint32) == dt.view(np.uint32) and lp["q"].view(np.uint32) == np.sqrt(dt).view(np.uint32)
                assert lp["hdt"] == np.float32(0.5) * dt and lp["h"] == np.float32(hh)
                want_rows = []
                for i in range(S):
                    times = [tg[i]] + ([tg[i] + dt] if stages == 2 else [])
                    for j, tj in enumerate(times):
                        r = lp["row_of"][i, j]
                        assert 0 <= r < len(rows) and rows[r].view(np.uint32) == np.float32(tj).view(np.uint32), (form, last, n, i, j)
                        if not want_rows or want_rows[-1].view(np.uint32) != np.float32(tj).view(np.uint32):
                            want_rows.append(np.float32(tj))
                    if stages == 2 and i + 1 < S and (tg[i] + dt).view(np.uint32) != tg[i + 1].view(np.uint32):
                        differ += 1     # t_i + dt is not t[i + 1]: two rows
                        assert lp["row_of"][i, 1] != lp["row_of"][i + 1, 0]
                if last is None:
                    assert lp["last_row"] == -1
                else:
                    assert rows[lp["last_row"]].view(np.uint32) == np.float32(t1).view(np.uint32)
                    if want_rows[-1].view(np.uint32) != np.float32(t1).view(np.uint32):
                        want_rows.append(np.float32(t1))
                assert np.array_equal(rows.view(np.uint32), np.array(want_rows, dtype=np.float32).view(np.uint32))
                # evaluation count: every (step, stage) and the last step is one evaluation
                assert lp["row_of"].size + (last is not None) == R.n_evaluations(method, last, n)
                # coefficients: within 1 fp32 ulp of the fp64 value; G = sqrtf(2 D) in fp32, bit for bit
                cf = lp["coef"].view(np.float32)
                for r, tau in enumerate(rows):
                    Rr, iV, D = R.coef64(path, form, norm, float(tau))
                    for name, got, want in (("R", cf[r, 0], Rr), ("iV", cf[r, 1], iV), ("D", cf[r, 2], D)):
                        if np.isfinite(want):
                            assert _ulp_distance(got, want) <= 1.0, (name, form, last, n, float(tau), got, want)
                    if np.isfinite(cf[r, 2]):
                        with np.errstate(invalid="ignore"):
                            assert cf[r, 3].view(np.uint32) == np.sqrt(np.float32(2) * cf[r, 2]).view(np.uint32)
                if last == "Tweedie":
                    al, _, sg, _, _ = R.path_terms(path, float(np.float32(t1)))
                    assert _ulp_distance(lp["c0"], 1 / al) <= 1.0 and _ulp_distance(lp["c1"], sg * sg / al) <= 1.0
    if method == "Heun":
        assert differ > 0   # (the n = 50 grids hold steps whose t_i + dt and t[i + 1] differ in the last bit)


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------------
def _raw_opts(**kw):
    from mdgen_amd import _lib as L
    d = dict(method=1, path=1, diffusion_form=2, last_step=1, n_points=6, diffusion_norm=1.0, last_step_size=0.04, sample_eps=0.0)
    d.update(kw)
    return L.SdeOpts(**d)


def _plan_rc(o):
    from mdgen_amd import _lib as L
    a, b = np.zeros(64, np.uint32), np.zeros((64, 4), np.uint32)
    ro, sc = np.zeros(64, np.int32), np.zeros(6, np.uint32)
    n, s, l = C.c_int32(), C.c_int32(), C.c_int32()
    return L.lib.mdgen_debug_sde_plan(C.byref(o), a.ctypes.data, b.ctypes.data, 64, C.byref(n), ro.ctypes.data, C.byref(s), C.byref(l),
                                      sc.ctypes.data)


def test_library_refusals():
    from mdgen_amd import _lib as L
    lib = L.lib
    sh = L.Shape(1, 8, 4)
    fake = C.c_void_p(4096)      # every refusal below is decided before any pointer is followed or any device call is made
    cond = L.Cond(mask=fake, start_rot=fake, start_trans=fake, x_cond=fake, x_cond_mask=fake, aatype=fake)
    nbytes = C.c_size_t()

    def sample(o, x=fake, noise=fake, stride=8 * 4 * 21, cd=cond):
        return lib.mdgen_sample_sde(None, C.byref(sh), C.byref(o) if o is not None else None, x, noise, stride,
                                    C.byref(cd) if cd is not None else None, fake, 1 << 30, 0, None)

    bad = [dict(method=0), dict(method=3), dict(path=2), dict(path=-1), dict(diffusion_form=6), dict(diffusion_form=-1),
           dict(last_step=4), dict(last_step=-1), dict(n_points=1), dict(n_points=0), dict(last_step_size=1.0),
           dict(last_step_size=-0.1), dict(last_step_size=float("nan")), dict(sample_eps=1.0),
           dict(diffusion_form=1, sample_eps=0.96),           # SBDM: t0 = 0.96 >= t1 = 1 - 0.04
           dict(diffusion_form=1, sample_eps=0.0),            # SBDM at sample_eps = 0: pi / (2 tan 0)
           dict(path=0, diffusion_form=1, sample_eps=0.0),
           dict(path=0, method=2, last_step=0),               # Linear, Heun, no last step: K2 at t = 1, sigma = 0
           dict(diffusion_norm=-1.0)]                         # sqrt of a negative diffusion
    for kw in bad:
        o = _raw_opts(**kw)
        assert _plan_rc(o) == -2, kw
        assert lib.mdgen_sde_workspace_bytes(None, C.byref(sh), C.byref(o), C.byref(nbytes)) == -2, kw
        assert sample(o) == -2, (kw, lib.mdgen_last_error())
    # the message of a non-finite coefficient names the coefficient and the time
    assert sample(_raw_opts(diffusion_form=1)) == -2
    msg = lib.mdgen_last_error().decode()
    assert "D (the diffusion)" in msg and "t = 0" in msg, msg
    assert sample(_raw_opts(path=0, method=2, last_step=0)) == -2
    msg = lib.mdgen_last_error().decode()
    assert "iV" in msg and "t = 1" in msg, msg
    # the same options are fine where the coefficient is not read, or with the margin
    assert _plan_rc(_raw_opts(diffusion_form=1, sample_eps=1e-3)) == 0
    assert _plan_rc(_raw_opts(path=0, method=2, last_step=0, sample_eps=1e-3)) == 0
    assert _plan_rc(_raw_opts(path=0, method=1, last_step=0)) == 0          # Euler-Maruyama never evaluates at t1 without a last step
    assert _plan_rc(_raw_opts(path=0, last_step=3, last_step_size=0.0)) == 0  # the Euler last step reads no coefficient at t = 1
    # null arguments
    ok = _raw_opts()
    assert sample(None) == -1 and sample(ok, x=None) == -1 and sample(ok, noise=None) == -1 and sample(ok, cd=None) == -1
    for missing in ("mask", "start_rot", "start_trans", "x_cond", "x_cond_mask", "aatype"):
        cd = L.Cond(mask=fake, start_rot=fake, start_trans=fake, x_cond=fake, x_cond_mask=fake, aatype=fake)
        setattr(cd, missing, None)
        assert sample(ok, cd=cd) == -1, missing
    assert lib.mdgen_sde_workspace_bytes(None, C.byref(sh), C.byref(ok), None) == -1
    assert lib.mdgen_sde_workspace_bytes(None, C.byref(sh), None, C.byref(nbytes)) == -1
    assert lib.mdgen_debug_sde_plan(None, None, None, 0, None, None, None, None, None) == -1
    # alignment and stride (a state of (1, 8, 4) x 21 = 672 floats)
    assert sample(ok, x=C.c_void_p(4100)) == -7 and sample(ok, noise=C.c_void_p(4104)) == -7
    assert sample(ok, stride=674) == -7 and b"multiple of 4" in lib.mdgen_last_error()
    assert sample(ok, stride=668) == -7 and b"below one state" in lib.mdgen_last_error()
    # a row buffer that is too small
    o = _raw_opts()
    a, b = np.zeros(2, np.uint32), np.zeros((2, 4), np.uint32)
    ro, sc = np.zeros(64, np.int32), np.zeros(6, np.uint32)
    n, s, l = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.mdgen_debug_sde_plan(C.byref(o), a.ctypes.data, b.ctypes.data, 2, C.byref(n), ro.ctypes.data, C.byref(s), C.byref(l),
                                    sc.ctypes.data) == -7 and n.value == 6


def test_python_surface_refuses_before_touching_a_gpu():
    from mdgen_amd import _lib as L
    from mdgen_amd.transport import Sampler, create_transport
    s = Sampler(create_transport(None, "GVP", "velocity"))
    with pytest.raises(L.MdgenError, match="error -2"):
        s.sample_sde()                                        # the reference's defaults: SBDM at sample_eps = 0
    with pytest.raises(ValueError):
        s.sample_sde(diffusion_form="quadratic")
    with pytest.raises(ValueError):
        s.sample_sde(sampling_method="Milstein", diffusion_form="sigma")
    with pytest.raises(ValueError):
        s.sample_sde(diffusion_form="sigma", last_step="Median")
    with pytest.raises(L.MdgenError, match="error -2"):
        s.sample_sde(diffusion_form="sigma", num_steps=1)
    with pytest.raises(L.MdgenError, match="error -2"):
        Sampler(create_transport(None, "Linear", "velocity")).sample_sde(sampling_method="Heun", diffusion_form="sigma", last_step=None)
    # create_transport keeps sample_eps (default 0); check_interval follows the reference with sde=True, and is (0, 1) without
    t = create_transport(None, "GVP", "velocity", sample_eps=1e-3)
    assert t.sample_eps == 1e-3 and create_transport(None).sample_eps == 0
    assert t.check_interval(0, 1e-3, sde=False, eval=True) == (0, 1) and t.check_interval() == (0, 1)
    assert t.check_interval(0, 1e-3, diffusion_form="SBDM", sde=True, eval=True, last_step_size=0.04) == (1e-3, 1 - 0.04)
    assert t.check_interval(0, 1e-3, diffusion_form="sigma", sde=True, eval=True, last_step_size=0.0) == (0, 1 - 1e-3)
    Sampler(t).sample_sde()                                   # with the margin the reference's defaults are accepted


def test_wrapper_options_are_checked_on_the_host():
    """NewMDGenWrapper._sde_opts needs no device: the defaults, the step count and the refusals of `sde={...}`."""
    from mdgen_amd import _lib as L
    from mdgen_amd.wrapper import SDE_DEFAULT_STEPS, SDE_DEFAULTS, NewMDGenWrapper
    import argparse
    w = NewMDGenWrapper.__new__(NewMDGenWrapper)
    w.args = argparse.Namespace(path_type="GVP")
    o = w._sde_opts("sde", None, None)
    assert (o.method, o.path, o.diffusion_form, o.last_step, o.n_points) == (1, 1, 2, 1, SDE_DEFAULT_STEPS + 1) and SDE_DEFAULT_STEPS == 49
    assert (o.diffusion_norm, o.last_step_size, o.sample_eps) == (1.0, 0.04, 0.0)
    assert SDE_DEFAULTS == dict(diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, sample_eps=0.0)
    o = w._sde_opts("sde_heun", 4, dict(last_step=None, diffusion_form="linear"))
    assert (o.method, o.diffusion_form, o.last_step, o.n_points) == (2, 3, 0, 5)
    for num_steps, sde in ((None, dict(diffusion_form="quadratic")), (None, dict(form="sigma")), (0, None), (None, dict(diffusion_form="SBDM"))):
        with pytest.raises(L.MdgenError):
            w._sde_opts("sde", num_steps, sde)


@pytest.mark.parametrize("cli", ["sim_inference", "tps_inference", "upsampling_inference"])
def test_cli_accepts_the_sde_options_and_refuses_bad_ones(cli, tmp_path):
    import importlib
    mod = importlib.import_module("mdgen_amd." + cli)
    base = ["--data_dir", str(tmp_path), "--synthetic"]
    entry = mod.parse_args if hasattr(mod, "parse_args") else mod.main
    for extra in (["--sampling_method", "sde", "--num_steps", "0"], ["--sampling_method", "sde", "--diffusion_form", "quadratic"],
                  ["--sampling_method", "sde_heun", "--last_step", "Median"], ["--sampling_method", "euler", "--diffusion_form", "sigma"],
                  ["--last_step_size", "0.1"]):
        with pytest.raises(SystemExit):
            entry(base + extra)
    a = mod.build_parser().parse_args(base + ["--sampling_method", "sde_heun", "--num_steps", "4", "--diffusion_form", "linear",
                                              "--diffusion_norm", "0.5", "--last_step", "none", "--last_step_size", "0.1",
                                              "--sample_eps", "0.001"])
    from mdgen_amd.sim_inference import sde_kwargs
    assert a.sampling_method == "sde_heun"
    assert sde_kwargs(a) == {"sde": dict(diffusion_form="linear", diffusion_norm=0.5, last_step=None, last_step_size=0.1, sample_eps=0.001)}
    assert sde_kwargs(mod.build_parser().parse_args(base + ["--sampling_method", "sde"])) == {"sde": {}}
    assert sde_kwargs(mod.build_parser().parse_args(base + ["--sampling_method", "rk4"])) == {}


# ---- 4: Sampler.sample_sde with a generic callable -------------------------------------------------------------------------------
def test_sampler_generic_callable_fp64_against_the_reference(gold):
    """The host loop of Sampler.sample_sde runs in fp64 here, but on the library's fp32 time grid and with its fp32-rounded
    coefficients (the reference's are fp64): each of the <= 11 evaluations takes a time and <= 4 coefficients that are off by at
    most 2^-24 relative, through maps whose derivatives in them are O(1) except SBDM's D ~ 1 / t near t0 = 1e-3 (D itself ~ 1e3, a
    relative error all the same).  11 x 5 x 2^-24 = 3.3e-6 bounds the first-order effect; the gate is 1e-5."""
    from mdgen_amd.transport import Sampler, create_transport
    init, noise = torch.from_numpy(gold["init"]), torch.from_numpy(gold["noise"])
    calls = []

    def model(x, t):
        assert t.shape == (x.shape[0],) and t.dtype == x.dtype
        calls.append(1)
        return R.toy(x, t)
    worst = 0.0
    for path, form, method, last, eps in CASES:
        fn = Sampler(create_transport(None, path, "velocity", sample_eps=eps)).sample_sde(
            sampling_method=method, diffusion_form=form, diffusion_norm=float(gold["diffusion_norm"]), last_step=last,
            last_step_size=float(gold["last_step_size"]), num_steps=int(gold["n_points"]))
        del calls[:]
        out = fn(init, model, noise=noise)
        assert out.shape == (1,) + init.shape and out.dtype == torch.float64
        assert len(calls) == R.n_evaluations(method, last, 6)
        e = rel_l2(out[-1], torch.from_numpy(gold[R.golden_key(path, form, method, last, eps)]))
        worst = max(worst, e)
        assert e <= 1e-5, (path, form, method, last, eps, e)
    print(f"Sampler.sample_sde (generic callable, fp64 on the library's fp32 plan) against the reference: worst rel-L2 {worst:.2e}")
    # the host loop is sde_ref's arithmetic on the library's bits, operation for operation, in fp32
    i32, n32 = init.float(), noise.float()
    for method, last, form in (("Euler", "Mean", "sigma"), ("Heun", "Tweedie", "decreasing"), ("Heun", None, "linear"), ("Euler", "Euler", "constant")):
        fn = Sampler(create_transport(None, "GVP", "velocity")).sample_sde(sampling_method=method, diffusion_form=form, last_step=last,
                                                                          num_steps=6)
        p = R.make_plan(method, "GVP", form, 1.0, last, 0.04, 6, 0.0, torch.float32, from_library=True)
        assert torch.equal(fn(i32, model, noise=n32)[-1], R.solve(_f, i32, n32, p, method, last)), (method, last, form)
    # without `noise` the draw is torch's: the same seed gives the same sample, another seed another
    fn = Sampler(create_transport(None, "GVP", "velocity")).sample_sde(diffusion_form="sigma", num_steps=6)
    torch.manual_seed(3)
    a = fn(init, model)
    torch.manual_seed(3)
    b = fn(init, model)
    torch.manual_seed(4)
    c = fn(init, model)
    assert torch.equal(a, b) and not torch.equal(a, c)


# ---- 5: dispatch plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,last", [("Euler", "Mean"), ("Heun", "Tweedie"), ("Euler", None)])
def test_one_step_launches_the_rk_samplers_network_classes(method, last):
    """Per view, one step launches the trunk classes one midpoint step launches, with k_sde_embed in k_rk_embed's place: no kernel
    form is reached that the dispatch registry does not cover already.  One elementwise update, and nothing else of the integrator."""
    from dispatch_registry import CASES as REG
    from mdgen_amd._lib import dispatch_plan, sde_dispatch_plan, sde_opts
    from test_dispatch_cpu import ipa_signature, registry_signatures
    known_ipa = set().union(*registry_signatures()[1].keys())
    o = sde_opts(method, "GVP", "sigma", 1.0, last, 0.04, 50, 0.0)
    evals = R.n_evaluations(method, last, 2)
    shapes = sorted({(c["B"], c["T"], c["L"], bool(c.get("tps"))) for c in REG if c["mode"] == "euler"})
    assert len(shapes) >= 8
    for B, T, L_, tps in shapes:
        rk = dispatch_plan(B, T, L_, mode=5, tps=tps)
        sd = sde_dispatch_plan(B, T, L_, o, tps=tps)
        assert sd["streams"] == 1 and [v["B"] for v in sd["views"]] == [v["B"] for v in rk["views"]]
        for vr, vs in zip(rk["views"], sd["views"]):
            want = {("sde_embed" if cls == "rk_embed" else cls): n // 2 * evals for cls, n in vr["classes"].items()}
            assert vs["classes"] == want, (B, T, L_, tps)
            assert vs["classes"]["sde_embed"] == evals and "embed" not in vs["classes"] and "rk_embed" not in vs["classes"]
        assert sd["integrator"] == {"ode_sde_update": 1}
        assert {k for k in sd["prepare"] if not k.startswith("ipa.")} == {k for k in rk["prepare"] if not k.startswith("ipa.")}
        assert ipa_signature(sd) <= known_ipa, (B, T, L_, tps, sorted(ipa_signature(sd) - known_ipa))


# ---- 6: exports -------------------------------------------------------------------------------------------------------------------
def test_exports_header_and_binding_agree():
    from mdgen_amd import _lib as L
    new = ["mdgen_sample_sde", "mdgen_sde_workspace_bytes", "mdgen_debug_sde_plan", "mdgen_debug_sde_dispatch_plan", "mdgen_debug_sde_stage"]
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    declared = set(re.findall(r"\b(mdgen_\w+)\s*\(", hdr))
    for n in new:
        assert n in L.EXPORTS and n in declared and hasattr(L.lib, n) and getattr(L.lib, n).argtypes is not None, n
    assert "typedef struct mdgen_sde_opts" in hdr and "#define MDGEN_ABI_VERSION 8" in hdr
    # the ctypes struct has the header's layout: five int32, padding, three doubles
    assert C.sizeof(L.SdeOpts) == 48 and L.SdeOpts.diffusion_norm.offset == 24 and L.SdeOpts.sample_eps.offset == 40
    assert [n for n, _ in L.SdeOpts._fields_] == re.findall(r"^\s+(?:int32_t|double)\s+(\w+);", hdr[hdr.index("typedef struct mdgen_sde_opts"):
                                                                                                   hdr.index("} mdgen_sde_opts;")], re.M)
    assert L.SDE_FORMS["inccreasing-decreasing"] == 5 and L.SDE_LAST_STEPS[None] == 0
