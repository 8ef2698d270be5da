"""torchdiffeq 0.2.x `dopri5` restated in torch, as the reference calls it (transport.py:408-451, integrators.py:74-113):
odeint(f, x0, linspace(0, 1, 50), method='dopri5', atol=[atol], rtol=[rtol])[-1] with f(t, x) = model(x, ones(B) t).
Sources restated: rk_common.py (RKAdaptiveStepsizeODESolver._before_integrate / _advance / _adaptive_step,
_runge_kutta_step, _interp_fit, _interp_evaluate), misc.py (_select_initial_step, _optimal_step_size, _rms_norm,
_PerturbFunc), dopri5.py (the Dormand-Prince-Shampine tableau, DPS_C_MID).

Mixed precision as there: state / stages / k fp32; time-like values (t0, dt, t1) fp64 -- here Python floats; atol / rtol
1-element fp64 tensors, so tolerances, norms and the error ratio are fp64; every time handed to the drift is fp32 (numpy
float32 here, passed as a Python float holding that value).  The norm is the RMS over the WHOLE state: one step size for the
whole batch.

A test helper, not a test module: `solve(drift, x0)` drives any drift(t, y) -> dy/dt (the oracle forward,
LatentMDGenModel.forward, a closed form)."""
from __future__ import annotations

from fractions import Fraction as Fr

import numpy as np
import torch

# dopri5.py, as fp64 expressions (cast to the state's dtype by the solver)
ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.]
BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
C_SOL = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
C_ERROR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 - -12231 / 42400,
           11 / 84 - 649 / 6300, -1. / 60.]
C_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
         187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]

# the same tableau in exact arithmetic (order-condition checks)
EXACT_BETA = [
    [Fr(1, 5)],
    [Fr(3, 40), Fr(9, 40)],
    [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
    [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
    [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)],
    [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)],
]
EXACT_ALPHA = [Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)]
EXACT_SOL = EXACT_BETA[5] + [Fr(0)]
EXACT_ERROR = [Fr(35, 384) - Fr(1951, 21600), Fr(0), Fr(500, 1113) - Fr(22642, 50085), Fr(125, 192) - Fr(451, 720),
               Fr(-2187, 6784) + Fr(12231, 42400), Fr(11, 84) - Fr(649, 6300), Fr(-1, 60)]
EXACT_MID = [Fr(6025192743, 30085553152) / 2, Fr(0), Fr(51252292925, 65400821598) / 2, Fr(-2691868925, 45128329728) / 2,
             Fr(187940372067, 1594534317056) / 2, Fr(-1776094331, 19743644256) / 2, Fr(11237099, 235043384) / 2]

f32 = np.float32


class Controller:
    """The step-size logic of rk_common.py / misc.py in Python floats (fp64) and numpy float32 (the fp32 casts)."""

    def __init__(self):
        self.t0, self.dt = 0.0, 0.0
        self.last_t0 = self.last_dt = self.last_t1 = 0.0
        self.done = False
        self.accepted = self.rejected = 0

    def probe(self, d0, d1):
        """_select_initial_step: h0 from d0 = rms(x0 / scale), d1 = rms(k1 / scale)."""
        if d0 < 1e-5 or d1 < 1e-5:
            self.h0, self.h0_f32 = float(f32(1e-6)), True     # torch.tensor(1e-6, dtype=y0.dtype)
        else:
            self.h0, self.h0_f32 = 0.01 * d0 / d1, False
        self.h0 = abs(self.h0)
        return f32(self.h0), f32(self.t0 + self.h0)             # coefficient of x0 + h0 k1 (fp32), the probe's model time

    def first_step(self, d1, d2n):
        d2 = abs(d2n / self.h0)
        if d1 <= 1e-15 and d2 <= 1e-15:
            if self.h0_f32:
                h1 = float(max(f32(1e-6), f32(self.h0) * f32(1e-3)))
            else:
                h1 = max(float(f32(1e-6)), self.h0 * 1e-3)
        else:
            h1 = (0.01 / max(d1, d2)) ** (1. / float(4 + 1))
        h1 = abs(h1)
        big = float(f32(100) * f32(self.h0)) if self.h0_f32 else 100 * self.h0
        self.dt = min(big, h1)

    def stage_times(self):
        """fp32 t0 + alpha dt; the alpha == 1 stages at nextafter(fp32(t0 + dt), -inf) (Perturb.PREV)."""
        t0, dt, t1 = f32(self.t0), f32(self.dt), f32(self.t0 + self.dt)
        return [np.nextafter(t1, f32(-np.inf)) if f32(a) == 1 else t0 + f32(a) * dt for a in ALPHA]

    def step(self, ratio):
        accept = ratio <= 1
        t1 = self.t0 + self.dt
        if accept:
            self.last_t0, self.last_dt, self.last_t1 = self.t0, self.dt, t1
            self.t0 = t1
            self.accepted += 1
            self.done = self.t0 >= 1.0
        else:
            self.rejected += 1
        if ratio == 0:
            f = 10.0
        else:
            dfac = 1.0 if ratio < 1 else 0.2
            f = min(10.0, max(0.9 / ratio ** (1.0 / 5.0), dfac))
        self.dt = self.dt * f
        return accept

    def dense_s(self):
        return f32((1.0 - self.last_t0) / (self.last_t1 - self.last_t0))


def rms(x):
    return x.abs().pow(2).mean().sqrt()


def dense(y0, y1, k, dt, s):
    """rk_common.py _interp_fit + _interp_evaluate: y0, y1 fp32 states, k (..., 7) the step's stages, dt fp32 0-dim, s fp32."""
    y_mid = y0 + k.matmul(dt * torch.tensor(C_MID, dtype=torch.float64).to(k)).view_as(y0)
    f0, f1 = k[..., 0], k[..., -1]
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
    b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
    c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
    d = dt * f0
    e = y0
    x = torch.tensor(float(s), dtype=y0.dtype, device=y0.device)
    total = e + x * d
    xp = x
    for coef in (c, b, a):
        xp = xp * x
        total = total + xp * coef
    return total


def solve(drift, x0, atol=1e-6, rtol=1e-3, max_steps=10000, replay=None):
    """`replay` (optional): accepted (t0, dt) steps of another solve to take instead of the controller's choices (rejected
    attempts do not change the state, so this reproduces that solve's arithmetic step for step).
    Returns {"x": state at t = 1, "steps": accepted (t0, dt), "accepted", "rejected", "nfe", and what the controller saw:
    "init": (d0, d1, rms((f1 - k1) / scale)), "ratios": the error ratio of every attempted step, "stage_times": fp32 per attempt,
    "probe": (coefficient, time), "dense_s"}.  drift(t, y): t a Python float holding an fp32 value."""
    dev, dtype = x0.device, x0.dtype
    atol_t = torch.tensor([atol], dtype=torch.float64, device=dev)
    rtol_t = torch.tensor([rtol], dtype=torch.float64, device=dev)
    ctl = Controller()
    nfe = 0
    y0 = x0
    f0 = drift(0.0, y0)
    nfe += 1
    scale = atol_t + torch.abs(y0) * rtol_t
    d0, d1 = float(rms(y0 / scale)), float(rms(f0 / scale))
    coef, th = ctl.probe(d0, d1)
    y1 = y0 + float(coef) * f0
    f1 = drift(float(th), y1)
    nfe += 1
    d2n = float(rms((f1 - f0) / scale))
    ctl.first_step(d1, d2n)
    out = {"init": (d0, d1, d2n), "probe": (coef, th), "ratios": [], "stage_times": [], "steps": []}
    beta = [torch.tensor(b, dtype=torch.float64).to(dtype) for b in BETA]
    c_err = torch.tensor(C_ERROR, dtype=torch.float64).to(dtype)
    while not ctl.done:
        if replay is not None:
            ctl.t0, ctl.dt = replay[ctl.accepted]
        if ctl.accepted + ctl.rejected >= max_steps:
            raise RuntimeError("max_steps exceeded")
        if not ctl.t0 + ctl.dt > ctl.t0:
            raise RuntimeError("underflow in dt")
        ts = ctl.stage_times()
        dt = torch.tensor(float(f32(ctl.dt)), dtype=dtype)
        k = torch.empty(*f0.shape, 7, dtype=dtype, device=dev)
        k[..., 0] = f0
        for i in range(6):
            yi = y0 + k[..., :i + 1].matmul((beta[i] * dt).to(dev)).view_as(f0)
            k[..., i + 1] = drift(float(ts[i]), yi)
        nfe += 6
        y1 = yi
        err = k.matmul((dt * c_err).to(dev))
        tol = atol_t + rtol_t * torch.max(y0.abs(), y1.abs())
        ratio = float(rms(err / tol))
        out["ratios"].append(ratio)
        out["stage_times"].append(ts)
        t_start, dt_used = ctl.t0, ctl.dt
        if ctl.step(0.0 if replay is not None else ratio):
            out["steps"].append((t_start, dt_used))
            if ctl.done:
                out["dense_s"] = ctl.dense_s()
                out["x"] = dense(y0, y1, k, dt.to(dev), ctl.dense_s())
                break
            y0, f0 = y1, k[..., 6].clone()
    out.update(accepted=ctl.accepted, rejected=ctl.rejected, nfe=nfe)
    return out
