"""Drop-in for the slice of `mdgen.transport` the sampler uses:
`create_transport(...)` -> `Sampler(transport).sample_ode(sampling_method='euler', num_steps=50)`
-> `fn(x0, model_fn, **kw)` (transport.py:408-451, integrators.py:74-114).

velocity prediction + GVP/Linear path => integration interval (t0, t1) = (0, 1) exactly
(transport.py:95-124, 561-563).  The fixed-grid solvers are provided here: Euler, midpoint, heun3 and rk4 (torchdiffeq's
fixed_grid.py); adaptive dopri5 is `LatentMDGenModel.sample_dopri5`; the SDE sampler and the likelihood path are outside
the accelerated hot path.
"""
from __future__ import annotations

from functools import partial

import torch


class Transport:
    def __init__(self, path_type="GVP", prediction="velocity"):
        if prediction != "velocity":
            raise NotImplementedError("only velocity prediction is on the accelerated path")
        if path_type not in ("GVP", "Linear"):
            raise NotImplementedError("only GVP / Linear paths (t0, t1 = 0, 1)")
        self.path_type, self.prediction = path_type, prediction
        self.train_eps = self.sample_eps = 0

    def check_interval(self, *a, **k):
        return 0, 1

    # ---- training target and loss, forward only (transport.py:126-189) ----------------------
    def sample(self, x1):
        """transport.py:126-136: x0 ~ N(0, I), t ~ U(0, 1) (velocity + GVP/Linear: t0, t1 = 0, 1), on x1's device."""
        x0 = torch.randn_like(x1)
        t = torch.rand((x1.shape[0],)).to(x1)
        return t, x0, x1

    def plan(self, t, x0, x1):
        """path.py:131-135 `plan`: (t, xt, ut) with xt = alpha x1 + sigma x0, ut = alpha' x1 + sigma' x0, computed by
        `mdgen_path_plan` (GVP: alpha = sin(pi t / 2), sigma = cos(pi t / 2); Linear: alpha = t, sigma = 1 - t)."""
        from ._lib import lib, launch, ptr, require_cuda
        x0 = x0.to(torch.float32).contiguous()
        x1 = x1.to(torch.float32).contiguous()
        t = t.to(torch.float32).contiguous()
        require_cuda(t, x0, x1)
        xt, ut = torch.empty_like(x1), torch.empty_like(x1)
        B = x1.shape[0]
        launch(lib.mdgen_path_plan, x1, B, x1.numel() // B, 1 if self.path_type == "GVP" else 0, ptr(t), ptr(x0), ptr(x1),
               ptr(xt), ptr(ut))
        return t, xt, ut

    def training_losses(self, model, x1, aatype1=None, mask=None, model_kwargs=None, t=None, x0=None):
        """transport.py:138-189 for the velocity model (non-design path): returns {'t', 'pred', 'loss'} with
        loss = mean_flat((model(xt, t) - ut)^2, mask).  `t` / `x0` may be given to reproduce a reference run
        (the reference draws them inside, :126-136).  Forward value only; the differentiated step is `mdgen_amd.train.Trainer.training_step`."""
        from ._lib import lib, launch, ptr, require_cuda
        model_kwargs = model_kwargs or {}
        if t is None or x0 is None:
            t_, x0_, _ = self.sample(x1)
            t = t_ if t is None else t
            x0 = x0_ if x0 is None else x0
        t, xt, ut = self.plan(t, x0, x1)
        pred = model(xt, t, **model_kwargs)
        if pred.shape != xt.shape:
            raise ValueError(f"model output {tuple(pred.shape)} != input {tuple(xt.shape)}")
        m = mask.to(torch.float32).expand_as(xt).contiguous()
        pred = pred.to(torch.float32).contiguous()
        require_cuda(pred, m)
        B = xt.shape[0]
        loss = torch.empty(B, device=xt.device, dtype=torch.float32)
        launch(lib.mdgen_masked_mse, xt, B, xt.numel() // B, ptr(pred), ptr(ut), ptr(m), ptr(loss))
        return {"t": t, "pred": pred, "loss": loss}


def create_transport(args=None, path_type="GVP", prediction="velocity", loss_weight=None, train_eps=None,
                     sample_eps=None):
    return Transport(path_type, prediction)


def linspace01(n):
    """The library's fp32 time grid (csrc/api.hip linspace01): ATen's linspace formula with every operation rounded by itself,
    t[i] = step * i below the midpoint and 1 - step * (n - 1 - i) from it on, step = 1 / (n - 1).  torch.linspace's CPU kernel
    contracts step * i into an FMA and differs from it in the last bit of a few entries (4 of 50 at n = 50)."""
    import numpy as np
    one = np.float32(1.0)
    step = one / np.float32(n - 1)
    return torch.from_numpy(np.array([step * np.float32(i) if i < n // 2 else one - step * np.float32(n - 1 - i)
                                      for i in range(n)], dtype=np.float32))


def rk_step(method, f, t0, t1, y0):
    """One step of torchdiffeq 0.2.x's fixed-grid `method` ("midpoint", "heun3", "rk4" -- the 3/8 rule) from (t0, y0) to t1, in
    y0's dtype; t0, t1 are 0-dim tensors of that dtype, f(t, y) the drift.  Operation for operation what csrc/ode.inc restates
    (fixed_grid.py Midpoint / Heun3 / RK4, rk_common.py rk3_step_func / rk4_alt_step_func)."""
    dt = t1 - t0
    third, two_thirds = (torch.tensor(1.0 / 3, dtype=y0.dtype, device=y0.device),
                         torch.tensor(2.0 / 3, dtype=y0.dtype, device=y0.device))
    k1 = f(t0, y0)
    if method == "midpoint":
        half_dt = 0.5 * dt
        k2 = f(t0 + half_dt, y0 + k1 * half_dt)
        return y0 + dt * k2
    if method == "heun3":
        k2 = f(t0 + dt * third, y0 + dt * (third * k1))
        k3 = f(t0 + dt * two_thirds, y0 + dt * (two_thirds * k2))
        return y0 + dt * (0.25 * k1 + 0.75 * k3)
    if method == "rk4":
        k2 = f(t0 + dt * third, y0 + (dt * k1) * third)
        k3 = f(t0 + dt * two_thirds, y0 + dt * (k2 - k1 * third))
        k4 = f(t1, y0 + dt * ((k1 - k2) + k3))
        return y0 + (((k1 + 3 * (k2 + k3)) + k4) * dt) * 0.125
    raise ValueError(f"unknown fixed-grid method {method!r}")


RK_METHODS = ("midpoint", "heun3", "rk4")


class Sampler:
    def __init__(self, transport: Transport):
        self.transport = transport

    def sample_ode(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, reverse=False):
        """Returns fn(x0, model_fn, **model_kwargs).  `num_steps` is the number of grid points
        (S = num_steps - 1 steps), as in the reference; `sampling_method`: "euler", "midpoint", "heun3" or "rk4", one step per
        grid interval (torchdiffeq's fixed-grid solvers).  The returned tensor holds only the final
        state, shape [1, *x0.shape], so that the caller's `[-1]` (wrapper.py:447) is unchanged."""
        if sampling_method != "euler" and sampling_method not in RK_METHODS:
            raise NotImplementedError(
                "Sampler.sample_ode implements the fixed-grid samplers (sampling_method='euler', 'midpoint', 'heun3', 'rk4'); "
                "adaptive dopri5 is NewMDGenWrapper.inference(..., sampling_method='dopri5') / LatentMDGenModel.sample_dopri5")
        if reverse:
            raise NotImplementedError("reverse-time sampling is not used by the wrapper")
        S = int(num_steps) - 1
        if sampling_method != "euler":
            if S < 1:
                raise ValueError(f"num_steps is the number of grid points: it must be >= 2, got {num_steps}")
            return self._sample_rk(sampling_method, S)

        def _sample(x0, model_fn, **model_kwargs):
            from .model import LatentMDGenModel
            fn, kw = model_fn, dict(model_kwargs)
            use_graph = kw.pop("use_graph", True)   # build-specific keyword: capture / replay the rollout as a hipGraph
            model_kwargs = dict(kw)
            if isinstance(fn, partial):
                kw = {**fn.keywords, **kw}
                fn = fn.func
            owner = getattr(fn, "__self__", None)
            if isinstance(owner, LatentMDGenModel) and getattr(fn, "__name__", "") in ("forward", "forward_inference"):
                return owner.sample_euler(x0, S, use_graph=use_graph, **kw)[None]
            # generic drift (any callable): explicit Euler on the host side, x stays on the device
            tg = torch.linspace(0, 1, S + 1)
            x = x0
            for i in range(S):
                t = torch.ones(x.shape[0], device=x.device) * tg[i]
                x = x + (tg[i + 1] - tg[i]) * model_fn(x, t, **model_kwargs)
            return x[None]

        return _sample

    @staticmethod
    def _sample_rk(method, S):
        def _sample(x0, model_fn, **model_kwargs):
            from .model import LatentMDGenModel
            fn, kw = model_fn, dict(model_kwargs)
            use_graph = kw.pop("use_graph", True)
            model_kwargs = dict(kw)
            if isinstance(fn, partial):
                kw = {**fn.keywords, **kw}
                fn = fn.func
            owner = getattr(fn, "__self__", None)
            if isinstance(owner, LatentMDGenModel) and getattr(fn, "__name__", "") in ("forward", "forward_inference"):
                return owner.sample_rk(x0, method, S, use_graph=use_graph, **kw)[None]
            # generic drift (any callable): the same formulas in a host loop, in the callable's dtype, on the library's fp32 grid
            tg = linspace01(S + 1).to(dtype=x0.dtype, device=x0.device)
            ones = torch.ones(x0.shape[0], dtype=x0.dtype, device=x0.device)
            x = x0
            for i in range(S):
                x = rk_step(method, lambda t, y: model_fn(y, ones * t, **model_kwargs), tg[i], tg[i + 1], x)
            return x[None]

        return _sample
