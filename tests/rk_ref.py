"""torchdiffeq 0.2.x's fixed-grid solvers `midpoint`, `heun3` and `rk4` (fixed_grid.py Midpoint / Heun3 / RK4 -- the 3/8 rule,
rk_common.py rk4_alt_step_func) as the reference's transport calls them (integrators.py:106-113: odeint(f, x0,
linspace(0, 1, S + 1), method=...)[-1]), restated in plain torch for any dtype and any drift callable.

A test helper, not a test module: the specification csrc/ode.inc and csrc/k_rk.hip are tested against.  Every line is one torch
operation, i.e. one rounded operation of the dtype, in the order the library's formulas are written in.  `third` and
`two_thirds` are 1.0 / 3 and 2.0 / 3 rounded to the dtype ((float)(1.0 / 3) in fp32).
"""
from __future__ import annotations

import numpy as np
import torch

METHODS = {"midpoint": 1, "heun3": 2, "rk4": 3}     # the C ABI's method codes
STAGES = {"midpoint": 2, "heun3": 3, "rk4": 4}
ORDER = {"midpoint": 2, "heun3": 3, "rk4": 4}


def _consts(dtype, device=None):
    return (torch.tensor(1.0 / 3, dtype=dtype, device=device), torch.tensor(2.0 / 3, dtype=dtype, device=device))


def grid(S, dtype=torch.float32, device=None):
    """t = linspace(0, 1, S + 1) in fp32, then cast: ATen's formula, t[i] = step * i below the midpoint and 1 - step * (S - i)
    from it on with step = 1 / S, every operation rounded by itself (the library's `linspace01`, the grid of its Euler sampler).
    torch.linspace's CPU kernel evaluates the same formula with step * i contracted into an FMA, which moves the last bit of a
    few entries (4 of 50 at S = 49); the grid is therefore written out here."""
    n = S + 1
    one = np.float32(1.0)
    step = one / np.float32(S)
    t = np.array([step * np.float32(i) if i < n // 2 else one - step * np.float32(S - i) for i in range(n)], dtype=np.float32)
    return torch.from_numpy(t).to(dtype=dtype, device=device)


def stage_times(method, t0, t1):
    """Model times of the stages of one step (0-dim tensors of the grid's dtype)."""
    dt = t1 - t0
    third, two_thirds = _consts(t0.dtype, t0.device)
    if method == "midpoint":
        return [t0, t0 + 0.5 * dt]
    if method == "heun3":
        return [t0, t0 + dt * third, t0 + dt * two_thirds]
    if method == "rk4":
        return [t0, t0 + dt * third, t0 + dt * two_thirds, t1]
    raise ValueError(method)


def stage_input(method, stage, y0, k, dt):
    """The state stage `stage` (0-based) is evaluated at, from y0 and the earlier velocities k[0 ..]."""
    third, two_thirds = _consts(y0.dtype, y0.device)
    if stage == 0:
        return y0
    if method == "midpoint":
        return y0 + k[0] * (0.5 * dt)
    if method == "heun3":
        return y0 + dt * (third * k[0]) if stage == 1 else y0 + dt * (two_thirds * k[1])
    if method == "rk4":
        if stage == 1:
            return y0 + (dt * k[0]) * third
        if stage == 2:
            return y0 + dt * (k[1] - k[0] * third)
        return y0 + dt * ((k[0] - k[1]) + k[2])
    raise ValueError(method)


def result(method, y0, k, dt):
    """y1 from y0 and the step's velocities."""
    if method == "midpoint":
        return y0 + dt * k[1]
    if method == "heun3":
        return y0 + dt * (0.25 * k[0] + 0.75 * k[2])
    if method == "rk4":
        return y0 + (((k[0] + 3 * (k[1] + k[2])) + k[3]) * dt) * 0.125
    raise ValueError(method)


def state(method, stage, y0, k, dt):
    """`stage_input` for stage < STAGES[method], `result` for stage == STAGES[method] (the numbering of mdgen_debug_rk_stage)."""
    return result(method, y0, k, dt) if stage == STAGES[method] else stage_input(method, stage, y0, k, dt)


def weights(method, stage):
    """The weights c_j with state = y0 + dt * sum_j c_j k_j in exact arithmetic (for error bounds)."""
    if stage == 0:
        return []
    table = {"midpoint": {1: [0.5], 2: [0.0, 1.0]},
             "heun3": {1: [1 / 3], 2: [0.0, 2 / 3], 3: [0.25, 0.0, 0.75]},
             "rk4": {1: [1 / 3], 2: [-1 / 3, 1.0], 3: [1.0, -1.0, 1.0], 4: [0.125, 0.375, 0.375, 0.125]}}
    return table[method][stage]


def step(method, f, t0, t1, y0):
    dt = t1 - t0
    ts = stage_times(method, t0, t1)
    k = []
    for j in range(STAGES[method]):
        k.append(f(ts[j], stage_input(method, j, y0, k, dt)))
    return result(method, y0, k, dt)


def solve(f, y0, method, S):
    """odeint(f, y0, linspace(0, 1, S + 1), method=method)[-1] in y0's dtype; f(t, y) with t a 0-dim tensor of that dtype."""
    t = grid(S, y0.dtype, y0.device)
    y = y0
    for i in range(S):
        y = step(method, f, t[i], t[i + 1], y)
    return y


def time_rows(method, S):
    """(fp32 bits of the time rows the library prepares for a solve, row index of every (step, stage)): the times of `stage_times`
    on the fp32 grid, in evaluation order; where the last stage of a step sits at t1 itself (rk4), the next step's first stage
    shares its row."""
    t = grid(S)
    rows, row_of = [], np.zeros((S, STAGES[method]), dtype=np.int64)
    shares = method == "rk4"
    for i in range(S):
        for j, tj in enumerate(stage_times(method, t[i], t[i + 1])):
            if j == 0 and i > 0 and shares:
                row_of[i, 0] = len(rows) - 1
                continue
            row_of[i, j] = len(rows)
            rows.append(tj)
    bits = torch.stack(rows).to(torch.float32).numpy().view(np.uint32)
    return bits, row_of
