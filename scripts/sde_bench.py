"""ms per network evaluation of the SDE sampler beside the fixed-grid samplers it shares its launches with:
sample_sde (Euler-Maruyama, 48 steps + the Mean last step: 49 evaluations), sample_rk (midpoint, 24 steps: 48 evaluations) and
sample_euler (49 steps), bf16 path, captured graphs, at B 16 x T 1000 x L 4 and at the ATLAS shape B 1 x T 250 x L 256.  Three rounds
of REPS solves per sampler, the samplers alternating within a round, hipEvent-timed after a warm-up solve (capture); prints one
JSON line per (shape, sampler).

    python scripts/sde_bench.py [--reps 5]
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
        samplers = {"sample_sde em48+mean": (49, lambda: w.model.sample_sde(zs, opts, noise=noise, **kw)),
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
        del w


if __name__ == "__main__":
    main()
