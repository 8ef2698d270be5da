"""The sampler's solver choice, stated once.  `resolve_solver` turns what a caller of `NewMDGenWrapper.inference()` / `upsample()` /
`rollout()` may say about the solver -- with the checkpoint's own `sampling_method` -- into one `SolverChoice`, or refuses; the three
methods dispatch on its `kind`.  `add_solver_arguments` / `solver_kwargs` are the same statement for the three command lines
(sim_inference, tps_inference, upsampling_inference).  Nothing here touches the GPU."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional

from .transport import RK_METHODS, SDE_METHODS

SOLVERS = ("euler", "dopri5") + RK_METHODS + SDE_METHODS
# Euler steps when num_steps is not given: the reference's hard-coded 50-point grid (wrapper.py:441-442)
EULER_DEFAULT_STEPS = 49
# steps of the fixed-grid Runge-Kutta solvers when num_steps is not given: 48 network evaluations each (Euler's default grid: 49)
RK_DEFAULT_STEPS = {"midpoint": 24, "heun3": 16, "rk4": 12}
# the SDE sampler's options when `sde={...}` does not name them.  The reference's own defaults (SBDM, 250 points) need
# sample_eps > 0; the "sigma" diffusion is finite on the whole interval with sample_eps = 0.  As many stochastic steps as Euler's
# default grid cost what that grid costs (+ 1 evaluation for the last step); their sample quality has not been measured.
SDE_DEFAULTS = dict(diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, sample_eps=0.0)
SDE_DEFAULT_STEPS = EULER_DEFAULT_STEPS


@dataclass(frozen=True)
class SolverChoice:
    kind: str                  # "euler" | "rk" | "dopri5" | "sde"
    method: str                # one of SOLVERS
    steps: Optional[int]       # fixed-grid / stochastic steps, defaults applied; None for dopri5
    atol: float
    rtol: float
    sde_opts: Any = None       # the checked `_lib.SdeOpts` of kind "sde"
    rng_seed: Optional[int] = None   # kind "sde": the kernels generate the noise from this seed (None: staged noise)


def sde_opts(sampling_method, num_steps, sde, path_type):
    """`_lib.SdeOpts` of `sampling_method` "sde" (Euler-Maruyama) / "sde_heun" with `num_steps` stochastic steps (default
    SDE_DEFAULT_STEPS) and the options of `sde` over SDE_DEFAULTS; an unknown option or value raises before anything runs."""
    from . import _lib as L
    unknown = set(sde or {}) - set(SDE_DEFAULTS)
    if unknown:
        raise L.MdgenError(f"sde options are {sorted(SDE_DEFAULTS)}, got {sorted(unknown)}")
    S = SDE_DEFAULT_STEPS if num_steps is None else int(num_steps)
    try:
        opts = L.sde_opts("Euler" if sampling_method == "sde" else "Heun", path_type, num_steps=S + 1, **{**SDE_DEFAULTS, **(sde or {})})
    except ValueError as e:
        raise L.MdgenError(str(e)) from None
    L.sde_plan(opts)   # (the library's own refusals: a non-finite coefficient, t0 >= t1)
    return opts


def resolve_solver(checkpoint_method, sampling_method=None, num_steps=None, atol=1e-6, rtol=1e-3, sde=None, path_type="GVP",
                   noise=None, rng_seed=None, rng_sample_base=0, rng_block_base=0) -> SolverChoice:
    """The solver of one call.  `checkpoint_method`: the checkpoint's `args.sampling_method`; the rest as `inference()` takes them.
    The reference samples with the checkpoint's method (argparse default 'dopri5', parsing.py:102) on the solver's own 50-point
    grid (wrapper.py:441): without an explicit choice (`sampling_method` / `num_steps`) a non-Euler checkpoint is refused instead of
    being silently sampled with a different solver."""
    from ._lib import MdgenError
    if sampling_method is not None and sampling_method not in SOLVERS:
        names = ", ".join(repr(n) for n in SOLVERS[:-1]) + f" or {SOLVERS[-1]!r}"
        raise MdgenError(f"sampling_method must be None, {names}, got {sampling_method!r}")
    if sampling_method == "dopri5" and num_steps is not None:
        raise MdgenError("num_steps sets the fixed Euler grid; dopri5 chooses its own steps (pass one or the other)")
    if num_steps is not None and int(num_steps) < 1:
        raise MdgenError(f"num_steps must be >= 1, got {num_steps}")
    if sampling_method is None and num_steps is None and checkpoint_method != "euler":
        raise MdgenError(f"checkpoint args say sampling_method={checkpoint_method!r}; pass sampling_method='dopri5' (CLI: "
                         "--sampling_method dopri5) for the reference's solver, or num_steps=... (CLI: --num_steps) "
                         "to sample with fixed-grid Euler")
    if sampling_method not in SDE_METHODS and (sde is not None or noise is not None):
        raise MdgenError("sde / noise are options of sampling_method='sde' | 'sde_heun'")
    if rng_seed is None and (rng_sample_base or rng_block_base):
        raise MdgenError("rng_sample_base / rng_block_base are indices of the generated noise: they go with rng_seed")
    if rng_seed is not None:
        if sampling_method not in SDE_METHODS:
            raise MdgenError("rng_seed is an option of sampling_method='sde' | 'sde_heun'")
        if noise is not None:
            raise MdgenError("rng_seed generates the noise in the kernels; noise supplies it (pass one or the other)")
        rng_seed = int(rng_seed)
        if int(rng_sample_base) < 0 or int(rng_block_base) < 0:
            raise MdgenError("rng_sample_base and rng_block_base must be >= 0")
    method = sampling_method or "euler"
    if method == "dopri5":
        return SolverChoice("dopri5", method, None, atol, rtol)
    if method in SDE_METHODS:
        opts = sde_opts(method, num_steps, sde, path_type)
        return SolverChoice("sde", method, opts.n_points - 1, atol, rtol, opts, rng_seed)
    default = RK_DEFAULT_STEPS[method] if method in RK_METHODS else EULER_DEFAULT_STEPS
    return SolverChoice("rk" if method in RK_METHODS else "euler", method, default if num_steps is None else int(num_steps), atol, rtol)


# ---- the command lines' solver options ---------------------------------------------------------------------------------------------
_SDE_OPTIONS = ("diffusion_form", "diffusion_norm", "last_step", "last_step_size", "sample_eps")


def _exit(message):
    raise SystemExit(message)


def add_solver_arguments(p, per="call"):
    """--num_steps, --sampling_method and the options of sde / sde_heun (Sampler.sample_sde's; unset ones take SDE_DEFAULTS)."""
    p.add_argument("--num_steps", type=int, default=None,
                   help=f"solver steps per {per} (Euler default: {EULER_DEFAULT_STEPS} = the reference's 50-point grid, Euler "
                        "checkpoints only; midpoint / heun3 / rk4 default: 24 / 16 / 12)")
    p.add_argument("--sampling_method", choices=list(SOLVERS), default=None,
                   help="solver (default: the checkpoint's, refused unless it is euler or --num_steps is given); dopri5: the "
                        "reference's adaptive solver, one step size per call shared by its batch; midpoint / heun3 / rk4: "
                        "fixed-grid solvers with --num_steps steps")
    p.add_argument("--diffusion_form", default=None,
                   choices=["constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing"],
                   help="sde / sde_heun: the diffusion coefficient's form (default sigma; SBDM needs --sample_eps > 0)")
    p.add_argument("--diffusion_norm", type=float, default=None, help="sde / sde_heun: the diffusion coefficient's magnitude (default 1)")
    p.add_argument("--last_step", default=None, choices=["Mean", "Tweedie", "Euler", "none"],
                   help="sde / sde_heun: the deterministic last step (default Mean)")
    p.add_argument("--last_step_size", type=float, default=None, help="sde / sde_heun: the last step's size (default 0.04)")
    p.add_argument("--sample_eps", type=float, default=None, help="sde / sde_heun: the interval's margin (default 0)")
    p.add_argument("--sde_seed", type=int, default=None,
                   help="sde / sde_heun: generate the noise inside the kernels from this seed (Philox; no staged noise buffer, "
                        "rollouts and upsampling in one graph; a peptide's noise does not depend on the rank that samples it)")


def sde_kwargs(args):
    """{} or {"sde": {...}} (with "rng_seed" for --sde_seed) from the SDE options; they go with sde / sde_heun only (else: SystemExit
    with the message, in all three command lines)."""
    given = {k: getattr(args, k, None) for k in _SDE_OPTIONS}
    given = {k: (None if k == "last_step" and v == "none" else v) for k, v in given.items() if v is not None}
    seed = getattr(args, "sde_seed", None)
    if getattr(args, "sampling_method", None) not in SDE_METHODS:
        named = list(given) + (["sde_seed"] if seed is not None else [])
        if named:
            _exit("--" + ", --".join(named) + ": options of --sampling_method sde / sde_heun")
        return {}
    return {"sde": given, **({} if seed is None else {"rng_seed": seed})}


def solver_kwargs(args, error=_exit):
    """The solver keywords of inference() / rollout() / upsample() from the options above; `error(message)` reports a refusal the
    way the command line at hand does and does not return.  No solver named: {"num_steps": ...} alone, so that a model whose
    methods predate `sampling_method` is still callable."""
    method, num_steps = getattr(args, "sampling_method", None), args.num_steps
    if method == "dopri5" and num_steps is not None:
        error("--num_steps sets the Euler grid; dopri5 chooses its own steps (pass one or the other)")
    if num_steps is not None and num_steps < 1:
        error(f"--num_steps must be >= 1, got {num_steps}")
    sde = sde_kwargs(args)
    if method is None:
        return {"num_steps": num_steps}
    return dict(num_steps=num_steps, sampling_method=method, **sde)
