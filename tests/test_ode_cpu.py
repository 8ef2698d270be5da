"""Host-only checks of the adaptive dopri5 sampler (mdgen_sample_dopri5, csrc/ode.inc): the torch restatement of torchdiffeq's
solver (tests/ode_ref.py) against closed forms and exact arithmetic, the library's step-size controller against it bit for bit
(mdgen_debug_dopri5_controller), and the kernels one attempted step launches (mdgen_debug_dispatch_plan mode 4)."""
import ctypes as C
import math
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import ode_ref as R


# ---- the tableau ---------------------------------------------------------------------------------------------------------
def _trees(max_order):
    """Rooted trees up to `max_order` (canonical nested tuples of subtrees)."""
    def canon(t):
        return tuple(sorted(canon(c) for c in t))

    def grow(t):
        out = [canon(t + ((),))]
        for i, c in enumerate(t):
            out += [canon(t[:i] + (g,) + t[i + 1:]) for g in grow(c)]
        return out
    levels = [{()}]
    for _ in range(max_order - 1):
        levels.append({g for t in levels[-1] for g in grow(t)})
    return [t for lv in levels for t in lv]


def _order(t):
    return 1 + sum(_order(c) for c in t)


def _gamma(t):
    g = _order(t)
    for c in t:
        g *= _gamma(c)
    return g


def _phi(A, t):
    """Elementary weights per stage: prod over children of A @ phi(child)."""
    n = len(A)
    v = [Fr(1)] * n
    for c in t:
        pc = _phi(A, c)
        v = [v[i] * sum(A[i][j] * pc[j] for j in range(n)) for i in range(n)]
    return v


def test_tableau_order_conditions_in_exact_arithmetic():
    A = [[Fr(0)] * 7] + [row + [Fr(0)] * (7 - len(row)) for row in R.EXACT_BETA]
    for i, a in enumerate(R.EXACT_ALPHA):
        assert sum(R.EXACT_BETA[i]) == a                      # rows sum to alpha
    trees = _trees(5)
    assert [sum(_order(t) == n for t in trees) for n in range(1, 6)] == [1, 1, 2, 4, 9]
    b4 = [s - e for s, e in zip(R.EXACT_SOL, R.EXACT_ERROR)]
    for t in trees:
        phi = _phi(A, t)
        assert sum(b * p for b, p in zip(R.EXACT_SOL, phi)) == Fr(1, _gamma(t)), t          # 5th order solution
        if _order(t) <= 4:
            assert sum(b * p for b, p in zip(b4, phi)) == Fr(1, _gamma(t)), t               # 4th order embedded
    assert sum(R.EXACT_MID) == Fr(1, 2)
    # the fp64 coefficients are the reference's expressions of the same numbers
    for x, e in zip(R.C_ERROR + R.C_MID, R.EXACT_ERROR + R.EXACT_MID):
        assert abs(x - float(e)) <= 1e-16 * max(1.0, abs(float(e)))


def test_dense_output_y_mid_is_fifth_order_on_exponential():
    # y' = y, y0 = 1: stages exact up to the tableau, y_mid vs exp(dt / 2) errs as O(dt^5)
    errs = []
    for dt in (0.1, 0.05):
        k = [Fr(0)] * 7
        y0 = Fr(1)
        dtf = Fr(dt)
        k[0] = y0
        for i in range(6):
            yi = y0 + dtf * sum(R.EXACT_BETA[i][j] * k[j] for j in range(i + 1))
            k[i + 1] = yi
        y_mid = y0 + dtf * sum(m * kj for m, kj in zip(R.EXACT_MID, k))
        errs.append(abs(float(y_mid) - math.exp(dt / 2)))
    assert errs[0] / errs[1] > 2 ** 4.5


# ---- ode_ref against closed forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [-1.5, 0.7, 3.0])
def test_linear_ode_matches_exp_within_rtol(lam):
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 5, 4, 7, generator=g) + 2.0
    res = R.solve(lambda t, y: lam * y, x0)
    want = x0.double() * math.exp(lam)
    err = float(((res["x"].double() - want).norm() / want.norm()))
    print(f"lam {lam}: rel err {err:.2e}, {res['accepted']} accepted, {res['rejected']} rejected, nfe {res['nfe']}")
    assert err < 5e-3
    assert res["nfe"] == 2 + 6 * (res["accepted"] + res["rejected"])
    t0, dt = res["steps"][-1]
    assert t0 < 1.0 <= t0 + dt and abs(sum(d for _, d in res["steps"]) - (t0 + dt)) < 1e-12


def test_dense_output_endpoints():
    g = torch.Generator().manual_seed(4)
    y0, y1 = torch.randn(3, 11, generator=g), torch.randn(3, 11, generator=g)
    k = torch.randn(3, 11, 7, generator=g)
    dt = torch.tensor(0.3)
    assert torch.equal(R.dense(y0, y1, k, dt, np.float32(0)), y0)
    assert torch.allclose(R.dense(y0, y1, k, dt, np.float32(1)), y1, rtol=0, atol=1e-4)


def _stiff_front(t, y):
    """A smooth start, then a sharp front at t = 0.6: the step grown on the smooth part is rejected there."""
    return torch.full_like(y, 40.0 / math.cosh(40.0 * (t - 0.6)) ** 2) - 0.1 * y


def test_a_sharp_front_forces_rejections():
    x0 = torch.linspace(-1, 1, 64).reshape(4, 16)
    res = R.solve(_stiff_front, x0)
    print(f"front: {res['accepted']} accepted, {res['rejected']} rejected")
    assert res["rejected"] >= 1
    assert res["nfe"] == 2 + 6 * (res["accepted"] + res["rejected"])
    assert torch.isfinite(res["x"]).all()


# ---- the library's controller, bit for bit -------------------------------------------------------------------------------
def _lib_controller(init, ratios, max_steps=1000):
    from mdgen_amd._lib import lib
    n = len(ratios)
    ini = (C.c_double * 3)(*init)
    rat = (C.c_double * max(n, 1))(*ratios)
    probe = (C.c_float * 2)()
    t0, dt = (C.c_double * max(n, 1))(), (C.c_double * max(n, 1))()
    bits = (C.c_uint32 * (6 * max(n, 1)))()
    acc = (C.c_int32 * max(n, 1))()
    ds = C.c_float()
    na = C.c_int32()
    rc = lib.mdgen_debug_dopri5_controller(ini, rat, n, max_steps, probe, t0, dt, bits, acc, C.byref(ds), C.byref(na))
    m = na.value
    return {"rc": rc, "probe": (np.float32(probe[0]), np.float32(probe[1])), "t0": list(t0[:m]), "dt": list(dt[:m]),
            "bits": [list(bits[6 * i:6 * i + 6]) for i in range(m)], "accept": list(acc[:m]), "dense_s": np.float32(ds.value)}


def _ref_controller(init, ratios):
    c = R.Controller()
    probe = c.probe(init[0], init[1])
    c.first_step(init[1], init[2])
    out = {"probe": probe, "t0": [], "dt": [], "bits": [], "accept": []}
    for r in ratios:
        out["t0"].append(c.t0)
        out["dt"].append(c.dt)
        out["bits"].append([int(np.float32(x).view(np.uint32)) for x in c.stage_times()])
        out["accept"].append(int(c.step(r)))
        if c.done:
            break
    out["done"] = c.done
    out["dense_s"] = c.dense_s() if c.done else None
    return out


def _assert_same(init, ratios):
    a, b = _lib_controller(init, ratios), _ref_controller(init, ratios)
    assert a["rc"] == (0 if b["done"] else 1)
    assert a["probe"][0].view(np.uint32) == np.float32(b["probe"][0]).view(np.uint32)
    assert a["probe"][1].view(np.uint32) == np.float32(b["probe"][1]).view(np.uint32)
    assert a["t0"] == b["t0"] and a["dt"] == b["dt"]          # fp64, exact
    assert a["bits"] == b["bits"] and a["accept"] == b["accept"]
    if b["done"]:
        assert a["dense_s"].view(np.uint32) == np.float32(b["dense_s"]).view(np.uint32)
    return b


def test_library_controller_replays_recorded_solves_bit_for_bit():
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 6, 3, 7, generator=g)
    seen_reject = seen_zero = False
    for drift in (lambda t, y: -1.5 * y, lambda t, y: 0.7 * y + torch.sin(torch.tensor(5 * t)), _stiff_front,
                  lambda t, y: torch.zeros_like(y)):        # (zero drift: d1 = 0 -> h0 = 1e-6 (fp32), error ratio 0)
        res = R.solve(drift, x0)
        b = _assert_same(res["init"], res["ratios"])
        assert b["done"] and len(b["accept"]) == len(res["ratios"])
        assert [s for s, a in zip(zip(b["t0"], b["dt"]), b["accept"]) if a] == res["steps"]
        assert b["bits"] == [[int(x.view(np.uint32)) for x in ts] for ts in res["stage_times"]]
        seen_reject |= res["rejected"] > 0
        seen_zero |= 0.0 in res["ratios"]
    assert seen_reject and seen_zero


def test_library_controller_on_hand_made_sequences():
    # accepted / rejected / growth-capped / ratio 0 / ratio exactly 1 / the h0 = 1e-6 and d1, d2 <= 1e-15 branches
    for init in ((1.0, 2.0, 1e-9), (0.16, 0.32, 1e-9), (3.0, 0.4, 0.05), (1e-7, 0.2, 0.01), (0.5, 1e-20, 1e-20)):
        for ratios in ([0.8] * 40, [0.0, 0.5, 2.0, 1.0, 0.99, 1.0000001, 0.3] + [0.7] * 60, [5.0, 3.0, 0.2] + [0.6] * 80):
            _assert_same(init, ratios)
    # landing exactly on t = 1: a first dt of 1 / n, kept by ratios in [0.9^5, 1) (factor max(0.9 ratio^-0.2, 1) = 1)
    for d0 in np.linspace(0.1, 2.0, 400):
        c = R.Controller()
        c.probe(float(d0), 0.2)
        c.first_step(0.2, 1e-9)
        if 1.0 / c.dt == round(1.0 / c.dt) and c.dt <= 0.5:
            break
    else:
        pytest.fail("no exactly representable first step found")
    b = _assert_same((float(d0), 0.2, 1e-9), [0.8] * 100)
    t0, dt = [x for x, a in zip(zip(b["t0"], b["dt"]), b["accept"]) if a][-1]
    assert t0 + dt == 1.0 and b["dense_s"] == 1.0
    # errors: a non-finite ratio, too many attempts
    assert _lib_controller((1.0, 2.0, 1e-3), [float("nan")])["rc"] == -9
    assert _lib_controller((1.0, 2.0, 1e-3), [5.0] * 50, max_steps=10)["rc"] == -10


# ---- what one attempted step launches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,L,tps", [(16, 1000, 4, False), (1, 250, 256, False), (8, 100, 4, True)])
def test_dispatch_plan_of_one_attempted_step(B, T, L, tps):
    from mdgen_amd._lib import dispatch_plan
    from test_dispatch_cpu import plan, registry_signatures, view_signatures, ipa_signature
    p = dispatch_plan(B, T, L, mode=4, tps=tps)
    assert p["integrator"] == {"ode_combine": 6, "ode_norm": 1}
    # one preparation for the six stage rows: adaLN table and fold pack once, no embedding-as-tail base rows
    assert p["prepare"]["adaln_table"] == 1 and p["prepare"].get("fold_pack", 1) == 1 and "embed_base" not in p["prepare"]
    assert len(p["views"]) == 1 and p["views"][0]["B"] == B
    cls = p["views"][0]["classes"]
    assert cls["embed"] == 6 and not any("+embed" in k for k in cls)        # six evaluations, every one embeds its own input
    tails = {k: v for k, v in cls.items() if k.startswith("mlp@fold+final") or k == "final_euler"}
    assert sum(tails.values()) == 6, cls                                     # the velocity comes out of each evaluation
    # every trunk form is one an oracle-backed GPU test covers: the view's set of classes is inside a registered signature
    trunk, ipa = registry_signatures()
    sig = next(iter(view_signatures(p)))
    assert any(sig <= s for s in trunk), (sig, list(trunk))
    # the same forms as a one-row preparation of the same shape (mdgen_denoiser_forward at B = 1 / Euler), six times over
    q = plan(B, T, L, "euler", S=2, tps=tps, options={"streams": 1})
    euler = {k: v for k, v in q["views"][0]["classes"].items()}
    for k in cls:
        if k != "embed":
            assert k.replace("+final", "") in {c.replace("+final+embed", "").replace("+final", "") for c in euler}, (k, euler)
