"""tests/golden/host_rounding.npz: the two values of the CPU fixtures that depend on the host that made them, recorded so that
tests/test_oracle_cpu.py checks the same thing on any host.

Run:  python oracle/gen_golden_host.py    (oracle only; on a host where `pytest tests/test_oracle_cpu.py` passes without this
file's entries, i.e. one whose BLAS code path reproduces the fixtures)

  train_grads_tps_rel7  -- the relative-frame 7-vectors (2, B, L, 7) of train_grads_tps.npz.  Their quaternion SIGN is whatever
                           LAPACK's eigh returns (rigid_utils.py:191-210), and that sign changes with the BLAS code path; it reaches
                           a Linear, so the loss and gradients depend on it.  (The forward fixtures store their own `rel7`.)
  rollout10_pre_omega0   -- the pre-omega angle of residue 0 (10, B, 1, 2) in the next-block torsions of the 10-block chain of
                           rollout10_sim.npz, as the oracle chains it.  It is built from the zero padding before the chain: a
                           degenerate frame, whose value is the host's last-bit rounding amplified to O(1), and the next block is
                           conditioned on it.  The test takes only this entry from here; every other torsion is the oracle's own.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_golden, weights_for   # noqa: E402
from oracle import mdgen_oracle as O             # noqa: E402


def rel7(start, end):
    iR, it = O.rigid_invert(*start)
    x_f = O.to_tensor_7(*O.rigid_compose(iR, it, *end))
    iR, it = O.rigid_invert(*end)
    x_r = O.to_tensor_7(*O.rigid_compose(iR, it, *start))
    return torch.stack([x_f, x_r])


def rollout10_pre_omega0():
    g = load_golden("rollout10_sim")
    cfg, sd = weights_for(g)
    cd = O.cfg_dict(cfg)
    cur = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    S, T = 10, g["S10_b0_zs"].shape[1]
    out = []
    for blk in range(10):
        ex = dict(cur)
        ex["torsions"] = cur["torsions"].expand(-1, T, -1, -1, -1)
        ex["trans"] = cur["trans"].expand(-1, T, -1, -1)
        ex["rots"] = cur["rots"].expand(-1, T, -1, -1, -1)
        atom14, _, _ = O.inference(sd, cd, ex, g[f"S{S}_b{blk}_zs"], S)
        cur = dict(cur, **O.rollout_glue(atom14[:, -1], cur["seqres"]))
        out.append(cur["torsions"][:, :, 0, 0])
    return torch.stack(out)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    g = load_golden("train_grads_tps")
    res = {"train_grads_tps_rel7": rel7((g["start_rot"], g["start_trans"]), (g["end_rot"], g["end_trans"])),
           "rollout10_pre_omega0": rollout10_pre_omega0()}
    path = os.path.join(ROOT, "tests", "golden", "host_rounding.npz")
    np.savez(path, **{k: v.numpy() for k, v in res.items()})
    print("wrote", path, {k: tuple(v.shape) for k, v in res.items()})
