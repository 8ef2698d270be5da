"""Outputs of the fused drivers on seeded inputs, for comparing two builds bit for bit (as `bench.py --dump-outputs` does for the
flagship inference() call): one rk4 rollout through `mdgen_rollout_rk` and one Euler upsampling through `mdgen_upsample_euler`, at
the smallest shapes of tests/test_rk_drivers_gpu.py and tests/test_upsampling_gpu.py (B 2, T 12, L 4; 3 blocks; key frames every 4;
3 steps), bf16 operands, captured graphs.  Run it once per build with that build's tree first on PYTHONPATH:

    PYTHONPATH=<tree> python scripts/dump_driver_outputs.py DIR

writes DIR/{rollout_rk,upsample_euler}_{atom14,samples}.npy and DIR/rollout_rk_next_{trans,rots,torsions}.npy."""
import os
import sys

import numpy as np
import torch


def main(out_dir):
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_batch, synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper, default_args
    torch.set_grad_enabled(False)
    dev = torch.device("cuda")
    B, T, L, R, c, S = 2, 12, 4, 3, 4, 3
    cfg = ModelConfig.forward_sim(num_frames=T, crop=4)
    sd = synth_state_dict(cfg, 9)
    out = {}

    w = NewMDGenWrapper(cfg, device=dev)
    w.model.load_state_dict(sd)
    zs = torch.randn(R, B, T, L, 21, generator=torch.Generator().manual_seed(5)).to(dev)
    atom14, nxt = w.rollout(synth_batch(B, 1, L, 0, dev, seed=31), T, R, num_steps=S, zs=zs, sampling_method="rk4", return_next=True)
    out.update(rollout_rk_atom14=atom14, rollout_rk_samples=w.last_samples)
    out.update({f"rollout_rk_next_{k}": nxt[k] for k in ("trans", "rots", "torsions")})

    args = default_args(cfg)
    args.cond_interval = c
    w = NewMDGenWrapper(args, device=dev)
    w.model.load_state_dict(sd)
    keys = [synth_batch(B, 1, L, 0, dev, seed=77 + k) for k in range(-(-T // c))]   # K different key frames per window
    kb = {k: torch.cat([f[k] for f in keys], 1) for k in ("torsions", "trans", "rots")}
    kb.update(seqres=keys[0]["seqres"], mask=keys[0]["mask"])
    z = torch.randn(B, T, L, 21, generator=torch.Generator().manual_seed(78)).to(dev)
    atom14, _ = w.upsample(kb, zs=z, num_steps=S)
    out.update(upsample_euler_atom14=atom14, upsample_euler_samples=w.last_samples)

    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    for name, t in out.items():
        a = t.float().cpu().numpy()
        assert np.isfinite(a).all(), name
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print("wrote", sorted(out), "to", out_dir)


if __name__ == "__main__":
    main(sys.argv[1])
