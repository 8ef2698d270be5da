"""Host-only checks of the fixed-grid Runge-Kutta samplers (midpoint, heun3, rk4; csrc/ode.inc, mdgen_amd/transport.py) against
tests/rk_ref.py: the observed order on a problem with a closed-form solution, the prepared time rows bit for bit, the dispatch plan
of one step against dopri5's, and the refusals that need no GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rk_ref as R

torch.set_grad_enabled(False)
METHODS = list(R.METHODS)


# ---- 1: observed order --------------------------------------------------------------------------------------------------------
A = torch.tensor([[-0.5, 2.0, 0.0], [-2.0, -0.5, 0.3], [0.0, -0.3, -1.0]], dtype=torch.float64)
Y0 = torch.tensor([[1.0, -0.7, 0.4]], dtype=torch.float64)


def _drift(y, t):
    """f(t, y) = (1 + 0.5 sin 3t) y A^T with the model's signature model(y, ones(B) t)."""
    return (1 + 0.5 * torch.sin(3 * t))[:, None] * (y @ A.T)


def _exact():
    integral = 1 + (1 - math.cos(3.0)) / 6      # of 1 + 0.5 sin 3t over [0, 1]
    return Y0 @ torch.linalg.matrix_exp(A * integral).T


@pytest.mark.parametrize("method", METHODS)
def test_observed_order_of_sample_ode(method):
    from mdgen_amd.transport import Sampler, create_transport
    s = Sampler(create_transport(None, "GVP", "velocity"))
    exact = _exact()
    err = {}
    for S in (16, 32):
        out = s.sample_ode(sampling_method=method, num_steps=S + 1)(Y0, _drift)
        assert out.shape == (1, 1, 3) and out.dtype == torch.float64
        err[S] = float((out[-1] - exact).norm())
        # the host loop is rk_ref's arithmetic, operation for operation
        assert torch.equal(out[-1], R.solve(lambda t, y: _drift(y, torch.ones(1, dtype=y.dtype) * t), Y0, method, S))
    order = math.log2(err[16] / err[32])
    print(f"{method}: err(16) {err[16]:.3e}, err(32) {err[32]:.3e}, observed order {order:.3f}")
    assert abs(order - R.ORDER[method]) <= 0.15


# ---- 2: time rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 12, 49])
@pytest.mark.parametrize("method", METHODS)
def test_time_rows_bit_for_bit(method, S):
    from mdgen_amd._lib import rk_plan
    bits, row_of = rk_plan(method, S)
    ref_bits, ref_row_of = R.time_rows(method, S)
    n = {"midpoint": 2 * S, "heun3": 3 * S, "rk4": 3 * S + 1}[method]
    assert bits.shape == (n,) and row_of.shape == (S, R.STAGES[method])
    assert np.array_equal(bits, ref_bits)
    assert np.array_equal(row_of, ref_row_of)
    # every (step, stage) maps to a row that holds its time
    t = R.grid(S)
    for i in range(S):
        for j, tj in enumerate(R.stage_times(method, t[i], t[i + 1])):
            want = np.float32(float(tj)).view(np.uint32)
            assert 0 <= row_of[i, j] < n and bits[row_of[i, j]] == want, (i, j)


# ---- 3: dispatch plan ---------------------------------------------------------------------------------------------------------
def _shapes():
    """(B, T, L, tps) of the sweep of tests/test_dispatch_cpu.py."""
    out = [(B, 1000, 4, False) for B in range(1, 17)]
    out += [(1, 250, L, False) for L in (8, 9, 16, 24, 33, 40, 64, 80, 96, 128, 160, 200, 256, 300, 400, 512, 724)]
    out += [(B, 100, 4, True) for B in (1, 8, 32, 64, 128, 256)]
    return out


@pytest.mark.parametrize("method", METHODS)
def test_one_step_launches_dopri5s_network_classes(method):
    """Per view, one step launches exactly what one dopri5 attempt launches per evaluation, with k_rk_embed in k_embed's place: no
    kernel form is reached that the dispatch registry does not cover already.  No norm launch, one elementwise update."""
    from mdgen_amd._lib import dispatch_plan
    from test_dispatch_cpu import ipa_signature, registry_signatures
    known_ipa = set().union(*registry_signatures()[1].keys())
    st = R.STAGES[method]
    for B, T, L_, tps in _shapes():
        d5 = dispatch_plan(B, T, L_, mode=4, tps=tps)
        rk = dispatch_plan(B, T, L_, mode=4 + R.METHODS[method], tps=tps)
        assert rk["streams"] == 1 and [v["B"] for v in rk["views"]] == [v["B"] for v in d5["views"]]
        for v5, vr in zip(d5["views"], rk["views"]):
            want = {}
            for cls, n in v5["classes"].items():
                assert n % 6 == 0, (cls, n)
                want["rk_embed" if cls == "embed" else cls] = n // 6 * st
            assert vr["classes"] == want, (B, T, L_, tps)
            assert vr["classes"]["rk_embed"] == st and "embed" not in vr["classes"]
        assert rk["integrator"] == {"ode_rk_update": 1}
        # the shared preparation: the IPA stack runs over rows x B x L tokens, in forms the registry's IPA entries cover
        assert {k for k in rk["prepare"] if not k.startswith("ipa.")} == {k for k in d5["prepare"] if not k.startswith("ipa.")}
        assert ipa_signature(rk) <= known_ipa, (B, T, L_, tps, sorted(ipa_signature(rk) - known_ipa))


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------
def test_library_refuses_unknown_method_and_no_steps():
    from mdgen_amd import _lib as L
    lib = L.lib
    sh = L.Shape(1, 8, 4)
    nbytes = C.c_size_t()
    bits = np.zeros(16, dtype=np.uint32)
    row_of = np.zeros(16, dtype=np.int32)
    n_rows, n_st = C.c_int32(), C.c_int32()
    for method, S in ((0, 4), (4, 4), (-1, 4), (3, 0), (1, -2)):
        assert lib.mdgen_rk_workspace_bytes(None, C.byref(sh), method, S, C.byref(nbytes)) == -2, (method, S)
        assert lib.mdgen_debug_rk_plan(method, S, bits.ctypes.data, 16, C.byref(n_rows), row_of.ctypes.data, C.byref(n_st)) == -2
        fake = C.c_void_p(4096)      # the method and the step count are judged before any pointer is followed
        cond = L.Cond(mask=fake, start_rot=fake, start_trans=fake, x_cond=fake, x_cond_mask=fake, aatype=fake)
        rc = lib.mdgen_sample_rk(None, C.byref(sh), method, S, fake, C.byref(cond), fake, 1 << 30, 0, None)
        assert rc == -2, (method, S, lib.mdgen_last_error())
    assert lib.mdgen_rk_workspace_bytes(None, C.byref(sh), 3, 4, None) == -1
    # a null argument gives -1: a NULL conditioning struct, and a struct with a NULL required field
    assert lib.mdgen_sample_rk(None, C.byref(sh), 3, 4, fake, None, fake, 1 << 30, 0, None) == -1
    for missing in ("mask", "start_rot", "start_trans", "x_cond", "x_cond_mask", "aatype"):
        cond = L.Cond(mask=fake, start_rot=fake, start_trans=fake, x_cond=fake, x_cond_mask=fake, aatype=fake)
        setattr(cond, missing, None)
        assert lib.mdgen_sample_rk(None, C.byref(sh), 3, 4, fake, C.byref(cond), fake, 1 << 30, 0, None) == -1, missing
    assert lib.mdgen_sample_rk(None, C.byref(sh), 3, 4, None, None, None, 0, 0, None) == -1
    with pytest.raises(L.MdgenError, match="error -2"):
        L.rk_plan("rk4", 0)
    with pytest.raises(L.MdgenError, match="error -2"):
        L.dispatch_plan(1, 8, 4, mode=8)


def test_python_surface_refuses_before_touching_a_gpu():
    from mdgen_amd.transport import Sampler, create_transport
    s = Sampler(create_transport(None, "GVP", "velocity"))
    with pytest.raises(NotImplementedError):
        s.sample_ode(sampling_method="rk5")
    with pytest.raises(ValueError):
        s.sample_ode(sampling_method="rk4", num_steps=1)     # one grid point: no step


@pytest.mark.parametrize("cli", ["sim_inference", "tps_inference", "upsampling_inference"])
def test_cli_refuses_zero_steps_and_unknown_methods(cli, tmp_path):
    import importlib
    mod = importlib.import_module("mdgen_amd." + cli)
    base = ["--data_dir", str(tmp_path), "--synthetic"]
    entry = mod.parse_args if hasattr(mod, "parse_args") else mod.main
    for extra in (["--sampling_method", "rk4", "--num_steps", "0"], ["--sampling_method", "rk5"], ["--num_steps", "0"]):
        with pytest.raises(SystemExit):
            entry(base + extra)
    for m in METHODS:
        assert mod.build_parser().parse_args(base + ["--sampling_method", m, "--num_steps", "4"]).sampling_method == m
