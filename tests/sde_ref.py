"""The SDE sampler's arithmetic (csrc/sde.inc, csrc/k_sde.hip) in torch, in a given dtype: the reference's Sampler.sample_sde
(transport.py:295-406, integrators.py:5-72, path.py) for a velocity model, restated with one model evaluation per (state, time) and
multiplications by R = alpha / alpha', iV = 1 / (sigma^2 - R sigma' sigma) in the divisions' place.  The coefficients are computed in
fp64 from the evaluation time (and rounded once to fp32 for an fp32 solve), or taken as bits from `mdgen_debug_sde_plan`."""
import numpy as np
import torch

METHODS = ("Euler", "Heun")
PATHS = ("GVP", "Linear")
FORMS = ("SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing")   # those the reference can run ("constant" raises there)
LAST_STEPS = ("Mean", None, "Tweedie", "Euler")
# state codes of mdgen_debug_sde_stage
X, NOISE, EM, PRED, HEUN, HEUN_NOISE, TWEEDIE, EULER, MEAN = range(9)


def toy(x, t):
    """The toy drift v(x, t) = tanh(x) (0.5 + t) - 0.3 x; t: (B,) or 0-dim."""
    t = t.reshape(-1, *([1] * (x.dim() - 1))) if t.dim() else t
    return torch.tanh(x) * (0.5 + t) - 0.3 * x


def interval(diffusion_form, last_step, last_step_size, sample_eps):
    """check_interval(..., sde=True) (transport.py:95-124) -> (t0, t1, h) as Python floats; h: the last step's size."""
    h = 0.0 if last_step is None else float(last_step_size)
    t0 = float(sample_eps) if diffusion_form == "SBDM" else 0.0
    t1 = 1.0 - float(sample_eps) if h == 0.0 else 1.0 - h
    return t0, t1, h


def grid(t0, t1, n, np_dtype):
    """th.linspace(t0, t1, n) by ATen's formula in `np_dtype`, every operation rounded by itself."""
    f = np_dtype
    start, end = f(t0), f(t1)
    step = (end - start) / f(n - 1)
    return np.array([start + step * f(i) if i < n // 2 else end - step * f(n - 1 - i) for i in range(n)], dtype=np_dtype)


def path_terms(path, t):
    """alpha, alpha', sigma, sigma', alpha' / alpha at t (a Python float), in fp64; a division by zero gives inf / nan, not an error."""
    with np.errstate(all="ignore"):
        t = np.float64(t)
        if path == "GVP":
            a = t * np.pi / 2
            return np.sin(a), np.pi / 2 * np.cos(a), np.cos(a), -np.pi / 2 * np.sin(a), np.pi / (2 * np.tan(a))
        return t, np.float64(1.0), 1 - t, np.float64(-1.0), np.float64(1.0) / t


def coef64(path, form, norm, tau):
    """(R, iV, D) at evaluation time tau, in fp64."""
    with np.errstate(all="ignore"):
        al, dal, sg, dsg, ar = path_terms(path, tau)
        t, norm = np.float64(tau), np.float64(norm)
        R = al / dal
        iV = 1 / (sg * sg - R * dsg * sg)
        D = {"constant": lambda: norm, "SBDM": lambda: norm * (ar * (sg * sg) - sg * dsg), "sigma": lambda: norm * sg,
             "linear": lambda: norm * (1 - t), "decreasing": lambda: 0.25 * (norm * np.cos(np.pi * t) + 1) ** 2,
             "inccreasing-decreasing": lambda: norm * np.sin(np.pi * t) ** 2}[form]()
        return R, iV, D


def make_plan(method, path, form, norm, last_step, last_step_size, n_points, sample_eps, dtype, from_library=False):
    """The times and coefficients of a solve as 0-dim tensors of `dtype`: {"t": [step][stage], "c": [step][stage] -> (R, iV, D, G),
    "t_last", "c_last", "dt", "q", "hdt", "h", "c0", "c1"}.  from_library: every value is the library's own fp32 value (exact in `dtype`)."""
    S, stages = n_points - 1, METHODS.index(method) + 1
    T = lambda v: torch.tensor(v, dtype=dtype)
    if from_library:
        from mdgen_amd import _lib as L
        lp = L.sde_plan(L.sde_opts(method, path, form, norm, last_step, last_step_size, n_points, sample_eps))
        rows, cf = lp["rows"].view(np.float32), lp["coef"].view(np.float32)
        at = lambda r: (T(float(rows[r])), tuple(T(float(x)) for x in cf[r]))
        steps = [[at(lp["row_of"][i, j]) for j in range(stages)] for i in range(S)]
        p = {k: T(float(lp[k])) for k in ("dt", "q", "hdt", "h", "c0", "c1")}
        p["t_last"], p["c_last"] = at(lp["last_row"]) if lp["last_row"] >= 0 else (None, None)
    else:
        f = np.float32 if dtype == torch.float32 else np.float64
        t0, t1, h = interval(form, last_step, last_step_size, sample_eps)
        tg = grid(t0, t1, n_points, f)
        dt = tg[1] - tg[0]

        def at(tau):
            R, iV, D = (f(x) for x in coef64(path, form, norm, float(tau)))
            with np.errstate(all="ignore"):
                G = np.sqrt(f(2) * D)
            return T(float(tau)), (T(float(R)), T(float(iV)), T(float(D)), T(float(G)))
        steps = [[at(tg[i])] + ([at(tg[i] + dt)] if stages == 2 else []) for i in range(S)]
        al, _, sg, _, _ = path_terms(path, float(f(t1)))
        p = {"dt": T(float(dt)), "q": T(float(np.sqrt(dt))), "hdt": T(float(f(0.5) * dt)), "h": T(float(f(h))),
             "c0": T(float(f(1 / al))), "c1": T(float(f(sg * sg / al)))}
        p["t_last"], p["c_last"] = at(f(t1)) if last_step is not None else (None, None)
    p["t"] = [[s[0] for s in st] for st in steps]
    p["c"] = [[s[1] for s in st] for st in steps]
    return p


def drift(v, x, c):
    """F(v, x; tau) = v + D * (((R * v) - x) * iV): velocity + diffusion * score."""
    R, iV, D, _ = c
    return v + D * (((R * v) - x) * iV)


def noise_term(xi, c, p):
    return c[3] * (xi * p["q"])


def state(code, p, step, x, v0=None, v1=None, xi=None):
    """State `code` (mdgen_debug_sde_stage) of step `step`, operation for operation what k_sde.hip computes."""
    c = p["c"][step]
    if code == X:
        return x
    if code == NOISE:
        return x + noise_term(xi, c[0], p)
    if code == EM:
        return (x + drift(v0, x, c[0]) * p["dt"]) + noise_term(xi, c[0], p)
    if code == PRED:
        return x + p["dt"] * drift(v0, x, c[0])
    if code in (HEUN, HEUN_NOISE):
        k1 = drift(v0, x, c[0])
        k2 = drift(v1, x + p["dt"] * k1, c[1])
        r = x + p["hdt"] * (k1 + k2)
        return r if code == HEUN else r + noise_term(xi, p["c"][step + 1][0], p)
    cl = p["c_last"]
    if code == MEAN:
        return x + drift(v0, x, cl) * p["h"]
    if code == TWEEDIE:
        return x * p["c0"] + p["c1"] * (((cl[0] * v0) - x) * cl[1])
    if code == EULER:
        return x + v0 * p["h"]
    raise ValueError(code)


LAST_CODE = {"Mean": MEAN, "Tweedie": TWEEDIE, "Euler": EULER}


def solve(f, x, noise, p, method, last_step):
    """The whole solve: f(t, x) the velocity model (t a 0-dim tensor), noise[i] step i's standard normals, p = make_plan(...)."""
    S = len(p["t"])
    for i in range(S):
        if method == "Euler":
            x = state(EM, p, i, x, f(p["t"][i][0], x), xi=noise[i])
        else:
            xh = state(NOISE, p, i, x, xi=noise[i])
            k1v = f(p["t"][i][0], xh)
            k2v = f(p["t"][i][1], state(PRED, p, i, xh, k1v))
            x = state(HEUN, p, i, xh, k1v, k2v)
    if last_step is None:
        return x
    return state(LAST_CODE[last_step], p, S - 1, x, f(p["t_last"], x))


def n_evaluations(method, last_step, n_points):
    return (METHODS.index(method) + 1) * (n_points - 1) + (0 if last_step is None else 1)


def golden_key(path, form, method, last_step, sample_eps):
    return f"{path}|{form}|{method}|{last_step}|{sample_eps:g}"


def golden_cases():
    """(path, form, method, last_step, sample_eps) of tests/golden/sde_toy.npz: the 80 combinations at sample_eps = 1e-3, and at 0 the
    non-SBDM ones with a last step."""
    out = []
    for eps in (1e-3, 0.0):
        for path in PATHS:
            for form in FORMS:
                for method in METHODS:
                    for last in LAST_STEPS:
                        if eps == 0.0 and (form == "SBDM" or last is None):
                            continue
                        out.append((path, form, method, last, eps))
    return out

