"""Writes tests/golden/sde_toy.npz: the reference's own Sampler.sample_sde in fp64 on the toy drift of tests/sde_ref.py.

Runs on the development machine only (it needs the reference checkout; pass its path or set MDGEN_REFERENCE) and is never imported
by a test.  `integrators.th.randn` is replaced by a function that hands out pre-drawn fp64 tensors, so the noise of every step is
an input of the golden file.  State (2, 3, 4, 21), 6 grid points; with sample_eps = 1e-3 all 80 combinations {GVP, Linear} x {SBDM,
sigma, linear, decreasing, inccreasing-decreasing} x {Euler, Heun} x {Mean, None, Tweedie, Euler}, with sample_eps = 0 the non-SBDM
ones that have a last step.  ("constant" raises TypeError in the reference; Heun on Linear without a last step at sample_eps = 0
is not finite there.)

    python scripts/gen_golden_sde.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, N_POINTS, LAST_STEP_SIZE, NORM = (2, 3, 4, 21), 6, 0.04, 1.0


def main(reference):
    sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), reference, os.path.join(ROOT, "tests")]
    import sde_ref as R
    from mdgen.transport import integrators
    from mdgen.transport.transport import Sampler, create_transport
    torch.set_default_dtype(torch.float64)
    gen = torch.Generator().manual_seed(20)
    init = torch.randn(SHAPE, generator=gen, dtype=torch.float64)
    noise = torch.randn((N_POINTS - 1,) + SHAPE, generator=gen, dtype=torch.float64)
    out = {"init": init.numpy(), "noise": noise.numpy(), "n_points": np.int64(N_POINTS), "last_step_size": np.float64(LAST_STEP_SIZE),
           "diffusion_norm": np.float64(NORM)}
    for path, form, method, last, eps in R.golden_cases():
        queue = list(noise)

        class Th:   # integrators.py sees `th.randn(x.size())`; everything else is torch's
            def __getattr__(self, name):
                return getattr(torch, name)

            @staticmethod
            def randn(size):
                xi = queue.pop(0)
                assert tuple(size) == tuple(xi.shape)
                return xi
        integrators.th = Th()
        transport = create_transport(None, path, "velocity")
        transport.sample_eps = eps   # (create_transport itself sets 0 for a velocity model whatever it is given)
        fn = Sampler(transport).sample_sde(
            sampling_method=method, diffusion_form=form, diffusion_norm=NORM, last_step=last, last_step_size=LAST_STEP_SIZE,
            num_steps=N_POINTS)
        calls = []

        def model(x, t):
            calls.append(float(t[0]))
            return R.toy(x, t)
        xs = fn(init, model)
        res = xs[-1]
        assert not queue and res.dtype == torch.float64 and bool(torch.isfinite(res).all()), (path, form, method, last, eps)
        # the reference evaluates the model twice per (state, time) where it needs drift and score: the times are sde_ref's, in pairs
        want = 2 * R.n_evaluations(method, None, N_POINTS) + {None: 0, "Mean": 2, "Tweedie": 1, "Euler": 1}[last]
        assert len(calls) == want, (len(calls), want)
        out[R.golden_key(path, form, method, last, eps)] = res.numpy()
    integrators.th = torch
    dst = os.path.join(ROOT, "tests", "golden", "sde_toy.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(out) - 5} results, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MDGEN_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    main(ref)
