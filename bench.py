"""bench.py -- sampled MD frames/sec of the MDGen denoising sampler on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one `NewMDGenWrapper.inference()` call on one batch of synthetic input resident in HBM:
noise zs (B,T,L,21) -> S fixed Euler steps of the denoiser -> atom14 (B,T,L,14,3)  (the region the
reference times at sim_inference.py:109-115).  Workload (BASELINE.json configs[1]): tetrapeptide
forward-sim, crop 4, 1000 frames, batch 16, bf16 MFMA operands, S = 49 Euler steps (the reference's
hard-coded 50-point grid, wrapper.py:441-442).  Batches shard over ranks with no data-path collective
(scaling = weak: every rank samples its own 16 x 1000 frames).

A plain run does what the headline figure needs and no more: set-up, W warm-up steps, the K timed steps, the dump if asked
for, the JSON line (`roofline`, `cpu_baseline` and `extra` are null in it).  `--full` adds the legs below, each a run of its own
after the timed steps (about half a minute in all); `--no-roofline`, `--no-cpu-baseline` and `--no-extra` take single ones out again.

With `--full` the JSON line also carries
  roofline     -- the dominant kernel (largest share of hipEvent time), its ALGORITHMIC flops per launch
                  divided by its average hipEvent-measured launch duration, vs the dense bf16 MFMA peak;
  cpu_baseline -- the CPU oracle (a port of the reference's PyTorch path, oracle/mdgen_oracle.py) timed on
                  this box's host cores on a bounded sample of the same workload;
  extra        -- (1 GPU, default workload) short legs for the other headline numbers, so that one bench line
                  carries them: ATLAS crop 256 x 250 frames (north_star's second target), the TPS shard of configs[2],
                  the reference CLI's own B = 1 shape, the 10-block rollout rate (the region sim_inference.py:109-115
                  times), one DDP-less training step of configs[4]'s per-GPU shape, and a box probe (HBM copy rate,
                  bf16 GEMM rate) that makes a slow box recognisable.

`--dump-outputs DIR` writes what the last timed step returned (float32 .npy files, see dump_outputs); the inputs are seeded,
so the files of two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0   # MI355X dense bf16 (MI355X_MICROARCH.md chip table)

WORKLOADS = {
    # name: (B, T, L, abs_pos_emb, n_pad)                 BASELINE.json configs[...]
    "tetrapeptide_fwdsim_crop4_T1000_B16": (16, 1000, 4, True, 0),      # [1] the headline (default)
    "atlas_crop256_T250_B1": (1, 250, 256, False, 16),                  # [3]
    "tetrapeptide_tps_crop4_T100_B32": (32, 100, 4, True, 0),           # [2]: batch 256 sharded over 8 GPUs = 32 / GPU
    "tetrapeptide_fwdsim_crop4_T100_B1": (1, 100, 4, True, 0),          # [0]'s shape
    "tetrapeptide_fwdsim_crop4_T1000_B1": (1, 1000, 4, True, 0),        # what the reference's CLI runs (B = 1)
    "tetrapeptide_fwdsim_crop4_T1000_B8": (8, 1000, 4, True, 0),    # working-set experiments (not bench lines)
    "tetrapeptide_fwdsim_crop4_T1000_B4": (4, 1000, 4, True, 0),
}


from mdgen_amd.synthetic import synth_batch  # noqa: E402  (shared with `python -m mdgen_amd.train --synthetic`)


def algorithmic_flops(cls, B, T, L):
    """Algorithmic flops of ONE launch of a kernel class (SURVEY.md section 8(d) per-token figures x N).
    dh padding 24->32, masked keys and tile padding are NOT counted."""
    N, C = B * T * L, 384
    cls = cls.split("@")[0]       # "@p4" / "@p8": four- / eight-wave form of a panel kernel (same work)
    if cls == "flash_proj_T":     # k_flash_proj: tiled attention + out-projection + gated residual
        return 4.0 * N * C * (T + 1) + 2.0 * N * C * C
    if cls == "flash_proj_L":
        return 4.0 * N * C * (L + 1) + 2.0 * N * C * C
    if cls == "projL_qkvT":       # k_ln_qkv<false, true>: residue-axis out-projection + the temporal q, k, v projection
        return 2.0 * N * C * C + 2.0 * N * C * 3 * C
    if cls in ("ln_qkv_L", "ln_qkv_T"):
        return 2.0 * N * C * 3 * C
    if cls == "proj_T":
        return 2.0 * N * C * C
    if cls == "proj_L":
        return 2.0 * N * C * C + (4.0 * N * C * (L + 1) if L <= 8 else 0.0)   # + fused micro-attention
    if cls == "attn_L_fused":   # L == 4: LN -> QKV -> 5-key attention -> out-projection -> residual, one kernel
        return 2.0 * N * C * 3 * C + 4.0 * N * C * (L + 1) + 2.0 * N * C * C
    if cls == "flash_T":
        return 4.0 * N * C * (T + 1)
    if cls == "flash_L":
        return 4.0 * N * C * (L + 1)
    if cls == "mlp":
        return 16.0 * N * C * C
    if cls == "proj_mlp":   # temporal out-projection + MLP block in one row-owner kernel (k_mlp_rows<NW, true>)
        return 18.0 * N * C * C
    return None


def cpu_baseline(cfg, sd, B, T, L, S, n_pad, budget_s=20.0):
    """Time the CPU oracle (port of the reference's PyTorch path) on a bounded sample: B=1 of the same
    (T, L) workload, n NFEs (network evaluations) until ~budget_s is spent, then scale to frames/s at S
    steps: value = T / (t_nfe * S + t_prepost)."""
    from oracle import mdgen_oracle as O
    torch.set_grad_enabled(False)
    cd = O.cfg_dict(cfg)
    g = torch.Generator().manual_seed(1)
    q = torch.randn(1, 1, L, 4, generator=g)
    R = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True)).expand(1, T, L, 3, 3).contiguous()
    tr = torch.cumsum(2.2 * torch.randn(1, 1, L, 3, generator=g), 2).expand(1, T, L, 3).contiguous()
    ang = 6.283185307 * torch.rand(1, 1, L, 7, generator=g)
    tors = torch.stack([ang.sin(), ang.cos()], -1).expand(1, T, L, 7, 2).contiguous()
    mask = torch.ones(1, L)
    if n_pad:
        mask[:, L - n_pad:] = 0
    batch = {"torsions": tors, "torsion_mask": torch.ones(1, L, 7), "trans": tr, "rots": R,
             "seqres": torch.randint(0, 20, (1, L), generator=g), "mask": mask}
    zs = torch.randn(1, T, L, cfg.latent_dim, generator=g)
    t0 = time.time()
    prep = O.prep_batch(batch, cd)
    t_pre = time.time() - t0
    x, n, t_nfe_total = zs, 0, 0.0
    while n < S and (n == 0 or t_nfe_total + t_nfe_total / n < budget_s):
        t0 = time.time()
        v = O.forward(sd, cd, x, torch.ones(1) * (n / S), **prep["model_kwargs"])
        x = x + v / S
        t_nfe_total += time.time() - t0
        n += 1
    t0 = time.time()
    O.postprocess(x, prep["rigids"], batch["seqres"], cd)
    t_post = time.time() - t0
    t_nfe = t_nfe_total / n
    value = T / (t_nfe * S + t_pre + t_post)
    return {"value": round(value, 3), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle (fp32 PyTorch port of the reference path) B=1 T={T} L={L}: {n} network evaluations "
                      f"timed ({t_nfe:.3f} s each on {torch.get_num_threads()} threads, os.cpu_count()={os.cpu_count()}), "
                      f"scaled to S={S} Euler steps + pre/post"}


# kernel class (hipEvent profile name) -> substring of the rocprof kernel name
_KERNEL_OF_CLASS = {"mlp": "k_mlp", "proj_mlp": "k_mlp_rows", "flash_T": "k_flash<", "flash_L": "k_flash<", "ln_qkv_T": "k_ln_qkv<false",
                    "ln_qkv_L": "k_ln_qkv<true", "proj_T": "k_proj<0>", "proj_L": "k_proj<2>",
                    "attn_L_fused": "k_ln_qkv_attn4<true, false>", "attn_L_fused@h32": "k_ln_qkv_attn4<true, true>", "flash_proj_T": "k_flash_proj", "flash_proj_L": "k_flash_proj",
                    "projL_qkvT": "k_ln_qkv<false, true>",
                    # tagged classes name ONE kernel form (looked up before the untagged base class)
                    "mlp@fold": "k_mlp_rows<4, false, true, true>", "mlp@p4": "k_mlp<3, false>", "mlp@p8": "k_mlp8<false>",
                    "mlp@p8x3": "k_mlp8<false, 3>", "proj_mlp@p4": "k_mlp<3, true>", "proj_mlp@p8": "k_mlp8<true>",
                    "proj_mlp@p8x3": "k_mlp8<true, 3>", "ln_qkv_T@p8": "k_ln_qkv8<false, false>", "ln_qkv_T@p8x2": "k_ln_qkv8<true, false>", "ln_qkv_T@h32x2": "k_ln_qkv8<true, true>",
                    "flash_proj_T@q128": "k_flash_proj8", "flash_proj_T@q64": "k_flash_proj(", "flash_proj_L@q64": "k_flash_proj(",
                    "flash_proj_L@q128": "k_flash_proj8"}


def pmc_traffic(kernel_class, workload):
    """HBM bytes per launch of the dominant kernel.  PMC counters cannot be read from inside the benchmark
    process, so this is the figure measured with scripts/pmc_traffic.sh (rocprofv3 --pmc, separate FETCH_SIZE /
    WRITE_SIZE passes, gfx950 correction) and committed as profiles/pmc_traffic.json -- or None when that file
    does not cover this kernel and workload."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            m = json.load(f)
    except (OSError, ValueError):
        return None, None
    sub = _KERNEL_OF_CLASS.get(kernel_class) or _KERNEL_OF_CLASS.get(kernel_class.split("@")[0])
    kern = m.get("workloads", {}).get(workload, {}).get("kernels")
    if kern is None and m.get("workload") == workload:   # (round-1 layout of the file: one workload)
        kern = m.get("kernels")
    if not kern or not sub:
        return None, None
    # the MLP class has two kernels (row-owner k_mlp_rows for launches that fill the chip, panel k_mlp<3> otherwise): take the
    # one with the larger grid, i.e. the trunk's
    hits = [(v.get("grid_threads", 0), v) for name, v in kern.items() if sub in name]
    if hits:
        v = max(hits, key=lambda t: t[0])[1]
        return v["hbm_bytes_per_launch"], "profiles/pmc_traffic.json (" + m.get("method", "") + ")"
    return None, None


def _dominant(rep, B, T, L, workload):
    """roofline object of the kernel class with the largest share of hipEvent time (classes with known algorithmic flops)."""
    tot = sum(v["ms"] for v in rep.values())
    known = [k for k in rep if algorithmic_flops(k, B, T, L)]
    if not known:
        return None
    dom = max(known, key=lambda k: rep[k]["ms"])
    avg_ms = rep[dom]["ms"] / rep[dom]["count"]
    ach = algorithmic_flops(dom, B, T, L) / (avg_ms * 1e-3) / 1e12
    traffic, traffic_src = pmc_traffic(dom, workload)
    return {"kernel": dom, "bound": "mfma", "achieved": round(ach, 2), "peak": MFMA_BF16_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": traffic,
            # PMC counters cannot be read in-process: `traffic` is the committed rocprofv3 --pmc measurement of this kernel
            # class (scripts/pmc_traffic.sh -> profiles/pmc_traffic.json), a constant of the build, not of this run
            "traffic_source": traffic_src, "traffic_measured_in_run": False, "avg_launch_ms": round(avg_ms, 4), "launches": rep[dom]["count"],
            "share_of_event_time": round(rep[dom]["ms"] / tot, 3),
            "by_kernel_ms_per_call": {k: round(v["ms"], 3) for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}}


def whole_step_frac(rep, B, T, L, seconds_per_call):
    """Algorithmic flops of every launch of one call (classes with a known figure) / wall time of one call / dense bf16 MFMA peak."""
    fl = sum(algorithmic_flops(k, B, T, L) * v["count"] for k, v in rep.items() if algorithmic_flops(k, B, T, L))
    return round(fl / seconds_per_call / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4)


def box_probe(dev):
    """~0.2 s: sustained HBM copy rate and a library bf16 GEMM rate of THIS box (torch = plumbing here, not the product):
    round 2 saw boxes whose HBM-touching kernels ran 1.5x slower than the pool's norm with the same build."""
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)   # 1 GiB
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(8):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_tbs = 8 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e12
    del a, b
    m = torch.randn(8192, 8192, device=dev).to(torch.bfloat16)
    n = torch.randn(8192, 8192, device=dev).to(torch.bfloat16)
    (m @ n)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(8):
        m @ n
    e1.record()
    torch.cuda.synchronize()
    gemm_tf = 8 * 2 * 8192 ** 3 / (e0.elapsed_time(e1) * 1e-3) / 1e12
    return {"hbm_copy_TBps": round(copy_tbs, 2), "library_bf16_gemm_8192_TFLOPs": round(gemm_tf, 1),
            "device": torch.cuda.get_device_name(dev)}


def sampler_leg(workload, dev, steps, warmup, S, options, roofline=False, rollouts=0):
    """One workload through `inference()` (or, rollouts > 0, `rollout()`): frames/s with inputs resident in HBM."""
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper
    B, T, L, abs_pos, n_pad = WORKLOADS[workload]
    tps = "_tps_" in workload
    cfg = ModelConfig(crop=L, num_frames=T, abs_pos_emb=abs_pos, sim_condition=not tps, tps_condition=tps)
    w = NewMDGenWrapper(cfg, device=dev)
    w.model.load_state_dict(synth_state_dict(cfg, 0))
    for k, v in options.items():
        w.model.set_option(k, v)
    batch = synth_batch(B, T if not rollouts else 1, L, n_pad, dev, seed=100, tps=tps)
    g = torch.Generator().manual_seed(137)
    if rollouts:
        zs = torch.randn(rollouts, B, T, L, cfg.latent_dim, generator=g).to(dev)
        step = lambda: w.rollout(batch, T, rollouts, num_steps=S, zs=zs)
    else:
        zs = torch.randn(B, T, L, cfg.latent_dim, generator=g).to(dev)
        step = lambda: w.inference(batch, zs=zs, num_steps=S)[0]
    for _ in range(warmup):
        out = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert torch.isfinite(out).all(), workload
    frames = B * T * max(rollouts, 1)
    res = {"value": round(frames / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "steps": steps,
           "batch": B, "num_frames": T, "crop": L, "euler_steps": S}
    if rollouts:
        res["num_rollouts"] = rollouts
    if roofline and not rollouts:
        w.model.profile(True)
        step()
        rep = w.model.profile_report()
        w.model.profile(False)
        res["roofline"] = _dominant(rep, B, T, L, workload)
        res["whole_step_frac_of_mfma_peak"] = whole_step_frac(rep, B, T, L, dt)
    del w
    torch.cuda.empty_cache()
    return res


def training_leg(dev, reps=2, train_precision=32):
    """One training step (forward + backward + clip + Adam) at configs[4]'s per-GPU shape (ATLAS crop 256 x 250 frames,
    B = 1), no gradient exchange (1 GPU).  flops = 3 x the forward's algorithmic flops.  train_precision: 32 =
    fp32 operands (exact mode), 16 = bf16 operands in the linear layers / weight gradients (the reference's `medium`)."""
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.optim import Adam
    from mdgen_amd.synthetic import synth_state_dict, synth_forward_inputs
    from mdgen_amd.train import TrainableModel
    B, T, L = 1, 250, 256
    cfg = ModelConfig.atlas(num_frames=T, crop=L)
    inp = synth_forward_inputs(cfg, B, T, L, 16, 27)
    gen = torch.Generator().manual_seed(5)
    ut = torch.randn(B, T, L, cfg.latent_dim, generator=gen)
    lm = (torch.rand(B, T, L, cfg.latent_dim, generator=gen) > 0.1).float() * inp["mask"][..., None]
    tm = TrainableModel(cfg, dev).load_state_dict(synth_state_dict(cfg, 6))
    tm.model.set_option("train_precision", train_precision)
    args = (inp["x"].to(dev), inp["t"].to(dev), ut.to(dev), lm.to(dev), inp["mask"].to(dev),
            (inp["start_rot"].to(dev), inp["start_trans"].to(dev)), inp["x_cond"].to(dev), inp["x_cond_mask"].to(dev),
            inp["aatype"].to(dev))
    opt = Adam(tm.params, lr=1e-4, grad_clip=1.0)

    def step():
        tm.zero_grad()
        loss, _ = tm.forward_backward(*args)
        opt.step(tm.grads)
        tm.mark_updated()   # no hand-back: the training kernels read the flat parameter buffer
        return loss
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    assert torch.isfinite(loss).all()
    N, C = B * T * L, 384
    fwd = N * (6 * 21 * C + 5 * (32 * C * C + 4 * C * (L + 1) + 4 * C * (T + 1)))
    return {"workload": "atlas_train_crop256_T250_B1", "ms_per_step": round(dt * 1e3, 2), "frames_per_s": round(B * T / dt, 1),
            "TFLOPs": round(3 * fwd / dt / 1e12, 1), "steps": reps,
            "arithmetic": "fp32 operands (exact mode)" if train_precision == 32 else
                          "bf16 operands in linear layers / weight gradients, fp32 accumulate + master weights; rest fp32"}


def extra_legs(dev, options):
    ex = {}
    t0 = time.perf_counter()
    def run(name, fn):
        try:
            ex[name] = fn()
        except Exception as e:   # an extra leg must never take the headline number down with it
            ex[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
    run("box_probe", lambda: box_probe(dev))
    run("atlas_crop256_T250_B1", lambda: sampler_leg("atlas_crop256_T250_B1", dev, 4, 2, 49, options, roofline=True))
    # (the two small shapes: 40 ms per call, so five timed calls behind two warm-up calls cost nothing and settle the clocks)
    run("tetrapeptide_tps_crop4_T100_B32", lambda: sampler_leg("tetrapeptide_tps_crop4_T100_B32", dev, 5, 2, 49, options))
    run("tetrapeptide_fwdsim_crop4_T1000_B1", lambda: sampler_leg("tetrapeptide_fwdsim_crop4_T1000_B1", dev, 5, 2, 49, options))
    run("rollout_10_blocks_T1000_B16", lambda: sampler_leg("tetrapeptide_fwdsim_crop4_T1000_B16", dev, 1, 1, 49, options, rollouts=10))
    run("atlas_train_crop256_T250_B1", lambda: training_leg(dev, reps=4, train_precision=16))
    run("atlas_train_crop256_T250_B1_fp32", lambda: training_leg(dev, train_precision=32))
    ex["seconds"] = round(time.perf_counter() - t0, 1)
    return ex


def self_launch(n, argv, script=None, extra_env=None):
    """Re-execute this script under torch.distributed.run (--standalone, 127.0.0.1, N processes on this node) and return its
    exit status; the children's stdout (rank 0's JSON line) and stderr pass through."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1", f"--nproc-per-node={n}",
           "--local-addr", "127.0.0.1", script or os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, **(extra_env or {}))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on these hosts
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def dist_selftest(dev):
    """`--dist-selftest` (round-5 verdict, item 8): on a one-GPU box the N > 1 code of this file never runs -- so run it with ONE rank:
    RCCL process-group initialisation on a 127.0.0.1 store with the device bound, barrier, the three reductions of the multi-rank
    path on DEVICE tensors (forced: a group of one skips them otherwise), teardown.  Prints one JSON line."""
    import socket
    import torch.distributed as dist
    from mdgen_amd.sharding import gather_over_ranks, max_over_ranks, sum_over_ranks
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    t0 = time.perf_counter()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0, device_id=dev)
    dist.barrier()
    torch.cuda.synchronize()
    res = {"dist_selftest": "ok", "backend": dist.get_backend(), "world": dist.get_world_size(),
           "max": max_over_ranks(1.25, dist, dev, force=True), "sum": sum_over_ranks(2.5, dist, dev, force=True),
           "gather": gather_over_ranks(3.75, dist, dev, force=True)}
    dist.barrier()
    dist.destroy_process_group()
    res["seconds"] = round(time.perf_counter() - t0, 2)
    assert res["max"] == 1.25 and res["sum"] == 2.5 and res["gather"] == [3.75], res
    print(json.dumps(res))


def timed_region(step, steps, warmup, dist, sync):
    """The contract's timed region: W untimed warm-up steps, then exactly K steps bracketed by a barrier + device
    synchronisation on both sides.  Returns (last output, seconds incl. the wait for the slowest rank, this rank's own seconds)."""
    out = None
    for _ in range(warmup):
        out = step()
    if dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    sync()
    dt_own = time.perf_counter() - t0          # this rank's own K steps (before it waits for the others)
    if dist:
        dist.barrier()
    sync()
    return out, time.perf_counter() - t0, dt_own


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """`--dump-outputs DIR`: write each array as DIR/<name>.npy in float32.  Above DUMP_LIMIT_BYTES in all, every array is cut
    to the same fixed, seeded sample of its flattened elements (in index order), so that two builds stay comparable."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(v.numel() * 4 for v in arrays.values())
    for name, v in arrays.items():
        v = v.detach().to("cpu", torch.float32)
        if total > DUMP_LIMIT_BYTES:
            n = max(1, v.numel() * DUMP_LIMIT_BYTES // total)
            v = v.reshape(-1)[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(0))[:n].sort().values]
        np.save(os.path.join(out_dir, name + ".npy"), v.numpy())


def headline(a, world, B, T, L, S, dt, per_rank, use_graph, roof=None, cpu=None, extra=None, data=None):
    value = B * T * a.steps * world / dt
    return {
        "metric": "sampled MD frames/sec", "value": round(value, 2), "unit": "frames/s", "n_gpus": world,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" if a.precision == "bf16" else "f32",
        "data": data or "synthetic (seeded random-init weights, synthetic peptide frames/torsions, CPU-seeded noise)",
        "config": {"workload": a.workload, "batch_per_gpu": B, "num_frames": T, "crop": L,
                   "euler_steps": S, "hipgraph": use_graph, "parallelism": f"batch-sharded x{world}, no collective"},
        # every rank's own rate over its K steps and the fastest / slowest ratio: a straggler GPU shows up here
        "per_rank_frames_per_s": [round(v, 1) for v in per_rank],
        "rank_max_over_min": round(max(per_rank) / min(per_rank), 4),
        "roofline": roof, "cpu_baseline": cpu, "extra": extra,
    }


def fake_sampler_main(a, rank, world):
    """Test hook (tests/test_multiproc_cpu.py, no GPU): the launcher / rendezvous / barrier / max-over-ranks / JSON plumbing of a
    multi-rank run with the sampler replaced by a sleep of 10 ms x (rank + 1) per step and gloo in place of RCCL."""
    dist = None
    if world > 1:
        import torch.distributed as dist_
        dist_.init_process_group("gloo")
        dist = dist_
    B, T, L, _, _ = WORKLOADS[a.workload]
    from mdgen_amd.sharding import gather_over_ranks, max_over_ranks
    _, dt, dt_own = timed_region(lambda: time.sleep(0.01 * (rank + 1)), a.steps, a.warmup, dist, lambda: None)
    dt = max_over_ranks(dt, dist)
    per_rank = [B * T * a.steps / s for s in gather_over_ranks(dt_own, dist)]
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(headline(a, world, B, T, L, a.euler_steps, dt, per_rank, False, data="none (fake sampler: test hook)")))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="tetrapeptide_fwdsim_crop4_T1000_B16", choices=list(WORKLOADS))
    ap.add_argument("--euler-steps", type=int, default=49, help="Euler steps S per inference() call (reference: 49)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16",
                    help="operand precision of the GEMM family / attention (fp32 = tolerance mode, ~10x slower)")
    ap.add_argument("--streams", type=int, default=None, help="library option 'streams' (default 2; 1 = single stream)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline figure does not need: the roofline of the dominant "
                         "kernel, the CPU baseline and the extra legs (about half a minute more)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline leg")
    ap.add_argument("--no-extra", action="store_true",
                    help="with --full: skip the extra legs (ATLAS, TPS, B = 1, rollout, training step, box probe)")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="library run-time option (mdgen_ctx_set_option), e.g. mlp_path=1; repeatable")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0) as DIR/<name>.npy, float32: "
                         "atom14 and aa_out of inference(), and the sampled latents (wrapper.last_samples)")
    ap.add_argument("--fake-sampler", action="store_true", help=argparse.SUPPRESS)   # test hook, see fake_sampler_main
    ap.add_argument("--dist-selftest", action="store_true", help=argparse.SUPPRESS)  # one-rank RCCL self-test, see dist_selftest
    return ap


def legs_after_timing(a, rank, world):
    """The legs that run after the timed steps, as a set of names: none in a plain run, and with `--full` each of `roofline`
    (rank 0), `cpu_baseline` and `extra` (one process only; `extra` for the default bf16 workload only) unless its `--no-*`
    option is given."""
    legs = set()
    if not a.full or rank != 0:
        return legs
    if not a.no_roofline:
        legs.add("roofline")
    if world == 1 and not a.no_cpu_baseline:
        legs.add("cpu_baseline")
    if world == 1 and not a.no_extra and a.precision == "bf16" and a.workload == "tetrapeptide_fwdsim_crop4_T1000_B16":
        legs.add("extra")
    return legs


def main():
    ap = build_parser()
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    options = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in a.option}

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start N ranks of this script (one process per GPU) and relay rank 0's
        # JSON line, so the bare command and the torch.distributed.run command give the same single line
        raise SystemExit(self_launch(a.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: one process per GPU (torch.distributed.run --nproc-per-node {a.gpus})")
    if a.fake_sampler:
        return fake_sampler_main(a, rank, world)
    torch.set_grad_enabled(False)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if a.dist_selftest:
        return dist_selftest(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist_
        dist_.init_process_group("nccl", device_id=dev)
        dist = dist_

    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper

    B, T, L, abs_pos, n_pad = WORKLOADS[a.workload]
    S = a.euler_steps
    tps = "_tps_" in a.workload
    cfg = ModelConfig(crop=L, num_frames=T, abs_pos_emb=abs_pos, sim_condition=not tps, tps_condition=tps)
    sd = synth_state_dict(cfg, 0)
    w = NewMDGenWrapper(cfg, device=dev, precision=a.precision)
    w.model.load_state_dict(sd)
    if a.streams is not None:
        w.model.set_option("streams", a.streams)
    for k, v in options.items():
        w.model.set_option(k, v)
    batch = synth_batch(B, T, L, n_pad, dev, seed=100 + rank, tps=tps)   # every rank: its own peptides (weak scaling)
    zs = torch.randn(B, T, L, cfg.latent_dim, generator=torch.Generator().manual_seed(137 + rank)).to(dev)
    use_graph = not a.no_graph

    def step():
        return w.inference(batch, zs=zs, num_steps=S, use_graph=use_graph)

    (atom14, aa_out), dt, dt_own = timed_region(step, a.steps, a.warmup, dist, torch.cuda.synchronize)
    if a.dump_outputs and rank == 0:   # before anything below runs the sampler again
        dump_outputs(a.dump_outputs, {"atom14": atom14, "aa_out": aa_out, "samples": w.last_samples})
    from mdgen_amd.sharding import gather_over_ranks, max_over_ranks
    dt = max_over_ranks(dt, dist, dev)
    per_rank = [B * T * a.steps / s for s in gather_over_ranks(dt_own, dist, dev)]
    if not torch.isfinite(atom14).all():
        smp = w.last_samples
        bad_a = (~torch.isfinite(atom14)).nonzero()
        bad_s = (~torch.isfinite(smp)).nonzero()
        print(f"NONFINITE atom14 {len(bad_a)} samples {len(bad_s)}; first atom14 idx {bad_a[:5].tolist()}; "
              f"first samples idx {bad_s[:5].tolist()}", file=sys.stderr)
        if len(bad_a):
            b, t, l = bad_a[0][:3].tolist()
            print("  samples at that token:", smp[b, t, l].tolist(), file=sys.stderr)
            print("  batch rots/trans at (b,0,l):", batch["rots"][b, 0, l].tolist(), batch["trans"][b, 0, l].tolist(),
                  "seqres", int(batch["seqres"][b, l]), file=sys.stderr)
        again, _ = step()
        torch.cuda.synchronize()
        print("  re-run nonfinite:", int((~torch.isfinite(again)).sum()), file=sys.stderr)
        lay = w.model.workspace_layout(B, T, L, S, True)
        ws = next(iter(w.model._ws.values()))
        names = ["h", "qf", "kf", "vf", "obuf", "mod", "silu_t", "ipa_out", "h_ipa", "ipa_proj", "ipa_feat", "mask_bl", "rel7", "tgrid"]
        offs = [getattr(lay, n) for n in names] + [lay.total_bytes]
        for n, o, e in zip(names, offs[:-1], offs[1:]):
            if n in ("mod", "silu_t", "ipa_out", "h_ipa", "ipa_proj", "mask_bl", "tgrid", "h"):
                v = ws[o:e].view(torch.float32)
                if n == "tgrid":
                    v = v[:S]
                if n == "mask_bl":
                    v = v[:B * L]
                print(f"  ws.{n}: nonfinite {int((~torch.isfinite(v)).sum())} of {v.numel()} absmax {float(v[torch.isfinite(v)].abs().max()) if torch.isfinite(v).any() else float('nan'):.3e}", file=sys.stderr)
        eager, _ = w.inference(batch, zs=zs, num_steps=S, use_graph=False)
        torch.cuda.synchronize()
        print("  eager re-run nonfinite:", int((~torch.isfinite(eager)).sum()), file=sys.stderr)
        raise AssertionError("non-finite atom14")
    legs = legs_after_timing(a, rank, world)
    roof = None
    if "roofline" in legs:
        # per-kernel-class durations measured with hipEvents on the launch stream (eager pass, graphs bypassed);
        # fp32 tolerance mode: its kernels (csrc/k_fp32.hip) are not priced against the bf16 MFMA peak -> None
        w.model.profile(True)
        step()
        rep = w.model.profile_report()
        w.model.profile(False)
        roof = _dominant(rep, B, T, L, a.workload)
        if roof is not None:   # the whole call (all kernels, two streams, graph replay) against the same peak
            roof["whole_step_frac_of_mfma_peak"] = whole_step_frac(rep, B, T, L, dt / a.steps)
    cpu = None
    if "cpu_baseline" in legs:
        cpu = cpu_baseline(cfg, sd, B, T, L, S, n_pad)
    extra = None
    if "extra" in legs:
        del w
        torch.cuda.empty_cache()
        extra = extra_legs(dev, dict(options, **({"streams": a.streams} if a.streams is not None else {})))
        # The package runs this workload at its power limit (profiles/r06_experiments.txt #12), so the honest yardstick next to the
        # 2.5 PFLOP/s data-sheet peak is what the SAME box sustains on a pure dense bf16 GEMM under the same limit.
        gemm_tf = (extra.get("box_probe") or {}).get("library_bf16_gemm_8192_TFLOPs")
        if roof is not None and gemm_tf:
            roof["whole_step_frac_of_box_library_gemm"] = round(roof["whole_step_frac_of_mfma_peak"] * MFMA_BF16_PEAK_TFLOPS / gemm_tf, 4)
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(headline(a, world, B, T, L, S, dt, per_rank, use_graph, roof, cpu, extra)))

if __name__ == "__main__":
    main()
