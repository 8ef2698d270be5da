"""ms per network evaluation of the SDE sampler beside the fixed-grid samplers it shares its launches with:
sample_sde (Euler-Maruyama, 48 steps + the Mean last step: 49 evaluations), sample_rk (midpoint, 24 steps: 48 evaluations) and
sample_euler (49 steps), bf16 path, captured graphs, at B 16 x T 1000 x L 4 and at the ATLAS shape B 1 x T 250 x L 256.  Three rounds
of REPS solves per sampler, the samplers alternating within a round, hipEvent-timed after a warm-up solve (capture); prints one
JSON line per (shape, sampler).  The buffer path of sample_sde is timed twice per round (the second entry shows the run's own
spread) beside the generator path (`rng=`: the noise computed in the kernels, nothing staged).  Then, at the first shape, a 10-block
`rollout(sampling_method="sde")`: the host loop over staged noise against the fused driver (`rng_seed=`), wall time per rollout.

    python scripts/sde_bench.py [--reps 5] [--no-rollout]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-rollout", action="store_true")
    a = ap.parse_args()
    from mdgen_amd import _lib as L
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_batch, synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper
    dev = torch.device("cuda")
    torch.set_grad_enabled(False)
    for B, T, L_ in ((16, 1000, 4), (1, 250, 256)):
        cfg = ModelConfig(crop=L_, num_frames=T, abs_pos_emb=True, sim_condition=True, tps_condition=False)
        w = NewMDGenWrapper(cfg, device=dev, precision="bf16")
        w.model.load_state_dict(synth_state_dict(cfg, 0))
        batch = synth_batch(B, T, L_, 0, dev, seed=1)
        kw = dict(w.prep_batch(batch)["model_kwargs"])
        kw["mask"] = kw["mask"].contiguous()
        kw["end_frames"] = None
        zs = torch.randn(B, T, L_, cfg.latent_dim, device=dev)
        noise = torch.randn(48, B, T, L_, cfg.latent_dim, device=dev)
        opts = L.sde_opts("Euler", "GVP", "sigma", 1.0, "Mean", 0.04, 49, 0.0)
        rng = L.rng_words(1234).to(dev)
        samplers = {"sample_sde em48+mean": (49, lambda: w.model.sample_sde(zs, opts, noise=noise, **kw)),
                    "sample_sde em48+mean (again)": (49, lambda: w.model.sample_sde(zs, opts, noise=noise, **kw)),
                    "sample_sde em48+mean rng": (49, lambda: w.model.sample_sde(zs, opts, rng=rng, **kw)),
                    "sample_rk midpoint24": (48, lambda: w.model.sample_rk(zs, "midpoint", 24, **kw)),
                    "sample_euler 49": (49, lambda: w.model.sample_euler(zs, 49, **kw))}
        for _, fn in samplers.values():   # warm-up: capture
            fn()
        torch.cuda.synchronize()
        runs = {name: [] for name in samplers}
        for _ in range(3):                # three rounds, the samplers alternating within each
            for name, (evals, fn) in samplers.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.reps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                runs[name].append(t0.elapsed_time(t1) / a.reps / evals)
        for name, (evals, _) in samplers.items():
            print(json.dumps({"shape": [B, T, L_], "sampler": name, "evaluations": evals, "reps": a.reps,
                              "ms_per_evaluation": [round(r, 4) for r in runs[name]]}), flush=True)
        if (B, T, L_) == (16, 1000, 4) and not a.no_rollout:
            rollout_leg(w, cfg, B, T, L_, dev)
        del w, noise
        torch.cuda.empty_cache()


def rollout_leg(w, cfg, B, T, L_, dev, blocks=10, steps=48):
    """Wall time of a `blocks`-block sde rollout: host loop (staged noise, one graph per block) against the fused driver."""
    import time
    from mdgen_amd.synthetic import synth_batch
    first = synth_batch(B, 1, L_, 0, dev, seed=2)
    zs = torch.randn(blocks, B, T, L_, cfg.latent_dim, device=dev)
    legs = {"rollout sde host loop": {}, "rollout sde fused (rng_seed)": {"rng_seed": 1234}}
    times = {name: [] for name in legs}
    for rep in range(3):   # the first repetition captures
        for name, extra in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w.rollout(first, T, blocks, num_steps=steps, zs=zs, sampling_method="sde", **extra)
            torch.cuda.synchronize()
            if rep:
                times[name].append(round(time.perf_counter() - t0, 4))
    for name in legs:
        print(json.dumps({"shape": [B, T, L_], "leg": name, "blocks": blocks, "steps_per_block": steps, "seconds_per_rollout": times[name]}),
              flush=True)


if __name__ == "__main__":
    main()
