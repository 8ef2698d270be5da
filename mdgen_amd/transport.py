"""Drop-in for the slice of `mdgen.transport` the sampler uses:
`create_transport(...)` -> `Sampler(transport).sample_ode(sampling_method='euler', num_steps=50)`
-> `fn(x0, model_fn, **kw)` (transport.py:408-451, integrators.py:74-114).

velocity prediction + GVP/Linear path => the ODE's integration interval (t0, t1) = (0, 1) exactly
(transport.py:95-124, 561-563).  The fixed-grid solvers are provided here: Euler, midpoint, heun3 and rk4 (torchdiffeq's
fixed_grid.py); adaptive dopri5 is `LatentMDGenModel.sample_dopri5`.  `Sampler.sample_sde` is the reference's stochastic sampler
(transport.py:295-406, integrators.py:5-72: Euler-Maruyama or Heun, then a last step) -> `LatentMDGenModel.sample_sde`, one
captured graph; its interval follows `check_interval(..., sde=True)` with the transport's `sample_eps`.  The likelihood path is
outside the accelerated hot path.
"""
from __future__ import annotations

from functools import partial

import torch


class Transport:
    def __init__(self, path_type="GVP", prediction="velocity", sample_eps=0):
        if prediction != "velocity":
            raise NotImplementedError("only velocity prediction is on the accelerated path")
        if path_type not in ("GVP", "Linear"):
            raise NotImplementedError("only GVP / Linear paths (t0, t1 = 0, 1)")
        self.path_type, self.prediction = path_type, prediction
        self.train_eps, self.sample_eps = 0, (0 if sample_eps is None else sample_eps)

    def check_interval(self, train_eps=0, sample_eps=0, *, diffusion_form="SBDM", sde=False, reverse=False, eval=False,
                       last_step_size=0.0):
        """transport.py:95-124 for a velocity model on the GVP / Linear path: (0, 1) for the ODE; for the SDE t0 = eps with the
        SBDM diffusion (else 0) and t1 = 1 - last_step_size, or 1 - eps without a last step size."""
        if not sde:
            return (1, 0) if reverse else (0, 1)
        eps = sample_eps if eval else train_eps
        t0 = eps if diffusion_form == "SBDM" else 0
        t1 = 1 - eps if last_step_size == 0 else 1 - last_step_size
        return (1 - t0, 1 - t1) if reverse else (t0, t1)

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
    """`sample_eps` (default 0) is kept: the SDE sampler's SBDM diffusion needs it > 0."""
    return Transport(path_type, prediction, sample_eps)


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
SDE_METHODS = ("sde", "sde_heun")   # wrapper / CLI names of Sampler.sample_sde(sampling_method="Euler" | "Heun")


def sde_solve(f, x, noise, plan, method, last_step):
    """The arithmetic of `mdgen_sample_sde` (csrc/sde.inc) as a host loop in x's dtype: f(t, x) the velocity model (t a 0-dim
    tensor), noise[i] step i's standard normals, `plan` = `_lib.sde_plan(opts)` -- the library's fp32 time rows and coefficients.
    With F(v, x; c) = v + D (((R v) - x) iV):  Euler-Maruyama x <- (x + F dt) + G (xi q);  Heun xh = x + G (xi q), K1 = F(f(xh)),
    xp = xh + dt K1, K2 = F(f(xp); at t + dt), x <- xh + (0.5 dt) (K1 + K2);  then the last step at t1."""
    import numpy as np
    T = lambda v: torch.tensor(float(v), dtype=x.dtype, device=x.device)
    rows, coef = plan["rows"].view(np.float32), plan["coef"].view(np.float32)
    dt, q, hdt, h = (T(plan[k]) for k in ("dt", "q", "hdt", "h"))

    def at(r):
        return T(rows[r]), [T(c) for c in coef[r]]

    def F(v, x_, c):
        return v + c[2] * (((c[0] * v) - x_) * c[1])
    for i, step_rows in enumerate(plan["row_of"]):
        t, c = at(step_rows[0])
        if method == "Euler":
            x = (x + F(f(t, x), x, c) * dt) + c[3] * (noise[i] * q)
        else:
            xh = x + c[3] * (noise[i] * q)
            k1 = F(f(t, xh), xh, c)
            xp = xh + dt * k1
            t2, c2 = at(step_rows[1])
            x = xh + hdt * (k1 + F(f(t2, xp), xp, c2))
    if last_step is None:
        return x
    t, c = at(plan["last_row"])
    v = f(t, x)
    if last_step == "Mean":
        return x + F(v, x, c) * h
    if last_step == "Tweedie":
        return x * T(plan["c0"]) + T(plan["c1"]) * (((c[0] * v) - x) * c[1])
    return x + v * h


def owning_model(model_fn, model_kwargs):
    """What a sampler closure is asked to run: (owner, kw, use_graph, model_kwargs) with `owner` the `LatentMDGenModel` whose
    `forward` / `forward_inference` -- possibly inside a `functools.partial` -- `model_fn` is, and `kw` its merged keywords; owner
    None for a generic callable, which takes the returned `model_kwargs`.  `use_graph` is the build-specific keyword (capture /
    replay the solve as a hipGraph), popped from both."""
    from .model import LatentMDGenModel
    fn, kw = model_fn, dict(model_kwargs)
    use_graph = kw.pop("use_graph", True)
    model_kwargs = dict(kw)
    if isinstance(fn, partial):
        kw = {**fn.keywords, **kw}
        fn = fn.func
    owner = getattr(fn, "__self__", None)
    if not (isinstance(owner, LatentMDGenModel) and getattr(fn, "__name__", "") in ("forward", "forward_inference")):
        owner = None
    return owner, kw, use_graph, model_kwargs


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
            owner, kw, use_graph, model_kwargs = owning_model(model_fn, model_kwargs)
            if owner is not None:
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
            owner, kw, use_graph, model_kwargs = owning_model(model_fn, model_kwargs)
            if owner is not None:
                return owner.sample_rk(x0, method, S, use_graph=use_graph, **kw)[None]
            # generic drift (any callable): the same formulas in a host loop, in the callable's dtype, on the library's fp32 grid
            tg = linspace01(S + 1).to(dtype=x0.dtype, device=x0.device)
            ones = torch.ones(x0.shape[0], dtype=x0.dtype, device=x0.device)
            x = x0
            for i in range(S):
                x = rk_step(method, lambda t, y: model_fn(y, ones * t, **model_kwargs), tg[i], tg[i + 1], x)
            return x[None]

        return _sample

    def sample_sde(self, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean",
                   last_step_size=0.04, num_steps=250):
        """The reference's signature and defaults (transport.py:347-406).  Returns fn(init, model_fn, **model_kwargs); `num_steps`
        is the number of grid points: num_steps - 1 stochastic steps ("Euler": Euler-Maruyama, "Heun") on linspace(t0, t1,
        num_steps), then `last_step` ("Mean", "Tweedie", "Euler" or None) at t1.  The default SBDM diffusion needs a transport
        with sample_eps > 0 (`create_transport(..., sample_eps=1e-3)`): at 0 the plan is refused, as the reference's run ends in
        NaN.  Build-specific keywords of fn: `noise` ((num_steps - 1, *init.shape) standard normals; default: drawn with
        torch.randn on init's device), `use_graph`, and -- in `noise`'s place -- `rng_seed` [, `rng_sample_base`, `rng_block_base`]: the
        Philox noise of `mdgen_sample_sde_rng` (include/mdgen_amd.h), generated in the kernels for the library's model and by
        `mdgen_amd.philox.sde_noise`, the numpy restatement of the same stream, for any other callable (init: (B, T, L, D)).  The
        returned tensor holds only the final state, shape [1, *init.shape], as `sample_ode` returns."""
        from . import _lib as L
        opts = L.sde_opts(sampling_method, self.transport.path_type, diffusion_form, diffusion_norm, last_step, last_step_size,
                          num_steps, self.transport.sample_eps)
        plan = L.sde_plan(opts)   # (refuses here, before any model call, what the library would refuse)

        def _sample(init, model_fn, **model_kwargs):
            noise = model_kwargs.pop("noise", None)   # (`model_kwargs` is this call's own dict)
            seed = model_kwargs.pop("rng_seed", None)
            bases = model_kwargs.pop("rng_sample_base", 0), model_kwargs.pop("rng_block_base", 0)
            if seed is not None and noise is not None:
                raise L.MdgenError("rng_seed generates the noise; noise supplies it (pass one or the other)")
            owner, kw, use_graph, model_kwargs = owning_model(model_fn, model_kwargs)
            if owner is not None:
                rng = None if seed is None else owner._staged(("sde_rng",), dict(rng=((4,), torch.int64)),
                                                              dict(rng=L.rng_words(seed, *bases)))["rng"]
                return owner.sample_sde(init, opts, noise=noise, use_graph=use_graph, rng=rng, **kw)[None]
            # generic drift (any callable): the same formulas in a host loop, in init's dtype, on the library's grid and coefficients
            if seed is not None:
                from .philox import sde_noise
                S = opts.n_points - 1
                noise = torch.stack([torch.from_numpy(sde_noise(tuple(init.shape), seed, i, bases[1], bases[0])) for i in range(S)])
                noise = noise.to(device=init.device, dtype=init.dtype)
            if noise is None:
                noise = torch.randn((opts.n_points - 1,) + tuple(init.shape), dtype=init.dtype, device=init.device)
            ones = torch.ones(init.shape[0], dtype=init.dtype, device=init.device)
            return sde_solve(lambda t, x: model_fn(x, ones * t, **model_kwargs), init, noise, plan, sampling_method, last_step)[None]

        return _sample
