"""Forward-simulation driver, command-line compatible with the reference's `sim_inference.py:1-14`
(`--sim_ckpt --data_dir --suffix --pdb_id --num_frames --num_rollouts --out_dir --split`), plus

  --num_steps S      Euler steps per block (the reference samples with its checkpoint's `sampling_method`; a non-Euler
                     checkpoint is refused unless S or --sampling_method is given);
  --sampling_method {euler,dopri5,midpoint,heun3,rk4,sde,sde_heun}   the solver: dopri5 is the reference's adaptive default (torchdiffeq,
                     atol 1e-6, rtol 1e-3), a host loop over the blocks inside `rollout()` (one step size per block, shared by a
                     --batch group); euler without --num_steps takes the reference's 49-step grid; midpoint / heun3 / rk4 are
                     torchdiffeq's fixed-grid solvers with --num_steps steps (default 24 / 16 / 12 = 48 network evaluations),
                     all blocks of a group in one captured graph (`mdgen_rollout_rk`), each peptide of a --batch group solved as
                     if alone.  No flag: as before;
  --per_block        one `inference()` call per block from Python instead of the multi-block `rollout()`, whatever the solver;
  --batch N          peptides of equal length sampled together in one `inference()` call (the reference runs
                     B = 1, sim_inference.py:101-102; B = 16 is the regime BASELINE.json's metric is quoted on);
  --chunk_idx/--n_chunks   the reference's own sharding switches (tps_inference.py:17-18,160-161): this process
                     handles chunk `chunk_idx` of `n_chunks` of the split.  Under `torch.distributed.run`
                     (RANK / WORLD_SIZE in the environment) the chunk is further sharded over the ranks -- one
                     process per GPU, no data-path collective (mdgen_amd/sharding.py);
  --synthetic        seeded weights instead of --sim_ckpt;  --npy  also save the sampled array;
  --analyze          after each group is sampled, `mdgen_amd.analysis.analyze` runs on the device tensor against the peptide's
                     conditioning array (the MD trajectory `{data_dir}/{name}{suffix}.npy`): torsion JSDs and decorrelation curves,
                     `{out_dir}/analysis.pkl` = {name: result} at the end.  Its time is outside the reported frames/s and printed
                     on its own line.  --tica [--tica_lag N]  adds `analyze(tica=True)`'s entries; a peptide whose MD trajectory is
                     too short for the lag is named on stderr and keeps its torsion entries.  --msm  adds `analyze(msm=True)`'s
                     k-means / MSM / PCCA+ entries (and the tICA ones) with `analyze_peptide_sim`'s --msm_k, --msm_states,
                     --md_msm_lag, --msm_lag, --kmeans_seed, --no_traj_msm; a peptide whose MSM is refused is named likewise.
                     --ensemble  adds `mdgen_amd.ensemble.analyze_ensemble`'s dict (Cartesian ensemble statistics against the same
                     MD trajectory) under `analysis[name]["ensemble"]`, on the device tensor the sampler left there; --sasa (with
                     --probe, --sasa_points, --sasa_threshold, --sasa_atoms, as `analyze_ensembles`) adds its surface entries;
  --superpose        each written trajectory (PDB and --npy) is superposed on its own first frame over its existing atoms,
                     unweighted, on the device before it is formatted (`mdgen_ens_superpose`): the reference's
                     `traj.superpose(traj)`.  Off by default.

The rollout (sim_inference.py:61-98) stays on the device: each block's last frame becomes the next block's
conditioning frame through `mdgen_atom14_to_cond` (no D->H->D round trip).  Output, as the reference
(sim_inference.py:117-119): `{out_dir}/{name}.pdb`, a multi-model PDB of all sampled frames written by
`mdgen_amd.pdb.atom14_to_pdb` (byte-compatible with `mdgen.utils.atom14_to_pdb`).  `--xtc` (sim_inference.py:121-125, and part of
the README's own forward-simulation command, README.md:72) is accepted: the PDB is always written; where `mdtraj` imports, the
reference's four lines run as they stand (superposed trajectory -> `{name}.xtc`, the PDB cut to its first frame), where it does not
(this image) a warning says so and the multi-model PDB stays.  `--no_frames` / `--tps` select other models: rejected loudly.
"""
from __future__ import annotations

import argparse
import sys
import os
import time
from typing import Dict, List, Sequence

import numpy as np
import torch

from .solver import add_solver_arguments, sde_kwargs, solver_kwargs  # noqa: F401 (sde_kwargs stays importable from here)


# ---- work selection (pure host logic; covered by the CPU / gloo tests) -------------------------------------------
def select_names(all_names: Sequence[str], pdb_id: Sequence[str] = (), chunk_idx: int = 0, n_chunks: int = 1,
                 rank: int = 0, world: int = 1) -> List[str]:
    """Names this process samples: chunk `chunk_idx` of `np.array_split(names, n_chunks)` (tps_inference.py:160-161),
    then the contiguous shard of `rank` among `world` processes, then the `--pdb_id` filter (applied last, as the
    reference does inside its loop, :166-167)."""
    from .sharding import shard_list
    if not (0 <= chunk_idx < n_chunks):
        raise ValueError(f"chunk_idx {chunk_idx} outside 0..{n_chunks - 1}")
    chunk = [str(n) for n in np.array_split(np.array(list(all_names), dtype=object), n_chunks)[chunk_idx]]
    mine = shard_list(chunk, rank, world)
    return [n for n in mine if not pdb_id or n in pdb_id]


def group_batches(names: Sequence[str], seqres: Dict[str, str], batch: int) -> List[List[str]]:
    """Consecutive groups of at most `batch` names with EQUAL sequence length (one `inference()` call each);
    order of first appearance is kept so that outputs are reproducible."""
    by_len: Dict[int, List[str]] = {}
    for n in names:
        by_len.setdefault(len(seqres[n]), []).append(n)
    out = []
    for _, ns in by_len.items():
        out += [ns[i:i + batch] for i in range(0, len(ns), max(1, batch))]
    return out


def dist_env():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


# ---- batches ---------------------------------------------------------------------------------------------------
def get_batch(arr, seqres_str, device):
    """sim_inference.get_batch (:32-59): first MD frame -> conditioning batch (B=1)."""
    from .geometry import atom14_to_cond, restype_order
    a = torch.from_numpy(np.copy(arr[0:1]).astype(np.float32)).to(device)          # [1,L,14,3]
    seqres = torch.tensor([restype_order[c] for c in seqres_str], device=device)[None]
    c = atom14_to_cond(a, seqres)
    L_ = seqres.shape[1]
    return {"torsions": c["torsions"][:, None], "torsion_mask": c["torsion_mask"], "trans": c["trans"][:, None],
            "rots": c["rots"][:, None], "seqres": seqres, "mask": torch.ones(1, L_, device=device)}


def collate(batches):
    """Stack B = 1 batches of equal L along the batch dimension (what the reference's DataLoader would do)."""
    return {k: torch.cat([b[k] for b in batches], 0) for k in batches[0]}


def rollout(model, batch, num_frames, num_steps, zs=None, sampling_method=None, **solver):
    """sim_inference.rollout (:61-98) with the glue on the device.  `solver`: further keywords of inference() for a named method."""
    from .geometry import atom14_to_cond
    ex = dict(batch)
    ex["torsions"] = batch["torsions"].expand(-1, num_frames, -1, -1, -1)
    ex["trans"] = batch["trans"].expand(-1, num_frames, -1, -1)
    ex["rots"] = batch["rots"].expand(-1, num_frames, -1, -1, -1)
    if sampling_method is not None:   # (a model's inference() need not know the keyword when no solver is named)
        solver["sampling_method"] = sampling_method
    atom14, _ = model.inference(ex, zs=zs, num_steps=num_steps, **solver)
    if sampling_method == "dopri5":
        st = model.last_stats
        print(f"dopri5: {st['nfe']} network evaluations ({st['accepted']} accepted, {st['rejected']} rejected steps)")
    c = atom14_to_cond(atom14[:, -1], batch["seqres"])
    new = dict(batch)
    new["trans"], new["rots"], new["torsions"] = c["trans"][:, None], c["rots"][:, None], c["torsions"][:, None]
    return atom14, new


def make_group_batch(names, arrs, seqres, device):
    """One conditioning batch (B = len(names)) for a group of equal-length peptides."""
    return collate([get_batch(arrs[n], seqres[n], device) for n in names])


def sample_group(model, batch, args, sample_base=0):
    """`num_rollouts` chained blocks for one batch; returns atom14 [B, R*T, L, 14, 3].  `sample_base`: the index of the batch's
    first peptide within the split -- with --sde_seed the sample index of its generated noise, so that a peptide draws the same
    noise whichever rank or chunk samples it."""
    kw = solver_kwargs(args)   # (no solver named: num_steps alone -- a model's rollout() need not know the other keywords)
    if "rng_seed" in kw:
        kw["rng_sample_base"] = sample_base
    if hasattr(model, "rollout") and not getattr(args, "per_block", False):
        atom14 = model.rollout(batch, args.num_frames, args.num_rollouts, **kw)
        if kw.get("sampling_method") == "dopri5":
            for b, st in enumerate(model.last_stats):
                print(f"dopri5 block {b}: {st['nfe']} network evaluations ({st['accepted']} accepted, {st['rejected']} rejected steps)")
        return atom14
    out = []
    num_steps = kw.pop("num_steps")
    for b in range(args.num_rollouts):   # --per_block: one inference() call per block from Python, whatever the solver
        if "rng_seed" in kw:
            kw["rng_block_base"] = b
        atom14, batch = rollout(model, batch, args.num_frames, num_steps, **kw)
        out.append(atom14)
    return torch.cat(out, 1)


def require_xtc_writer():
    """`--xtc` is the reference's mdtraj post-processing (sim_inference.py:121-125).  A pipeline that asks for `{name}.xtc` must not
    find out after hours of sampling that none was written: without mdtraj the command is refused BEFORE anything is sampled
    (exit status 2); drop `--xtc` to get the multi-model PDB, which holds every frame."""
    try:
        import mdtraj  # noqa: F401
    except ImportError:
        print("error: --xtc needs mdtraj (the reference's dependency for the XTC file), which is not installed; "
              "run without --xtc to get the multi-model PDB with all frames", file=sys.stderr)
        raise SystemExit(2)


def write_xtc(pdb_path, xtc_path):
    """`--xtc` (sim_inference.py:121-125): superpose the sampled trajectory on its first frame, save it as XTC and cut the PDB to
    that frame (mdtraj: checked by require_xtc_writer before sampling starts)."""
    import mdtraj
    traj = mdtraj.load(pdb_path)
    traj.superpose(traj)
    traj.save(xtc_path)
    traj[0].save(pdb_path)
    return True


def run(args, model, device, names_seqres, rank=0, world=1, batch_fn=make_group_batch, sync=None, dist=None):
    """The driver proper (sim_inference.py:100-128), given a loaded model: select this process's peptides
    (chunk, rank shard, --pdb_id), group them into batches of equal length, sample every group, write
    `{out_dir}/{name}.pdb`.  `names_seqres`: ordered {name: sequence} of the whole split.  With `dist` (an
    initialised torch.distributed module) the ranks meet at a barrier before and after the timed region and the
    reported rate is whole-job frames / slowest rank's time -- no collective touches sample data."""
    from .geometry import restype_order
    from .pdb import atom14_to_pdb
    from .sharding import max_over_ranks, sum_over_ranks
    sync = sync or (lambda: None)
    if getattr(args, "xtc", False):
        require_xtc_writer()
    names = select_names(list(names_seqres), args.pdb_id, args.chunk_idx, args.n_chunks, rank, world)
    seqres = {n: names_seqres[n] for n in names}
    split_index = {n: i for i, n in enumerate(names_seqres)}
    os.makedirs(args.out_dir, exist_ok=True)
    total_frames, total_s = 0, 0.0
    analysis, analysis_s = {}, 0.0
    if dist is not None:
        dist.barrier()
    for group in group_batches(names, seqres, args.batch):
        arrs = {n: np.lib.format.open_memmap(f"{args.data_dir}/{n}{args.suffix}.npy", "r") for n in group}
        batch = batch_fn(group, arrs, seqres, device)
        sync()
        start = time.time()
        all_atom14 = sample_group(model, batch, args, **({} if getattr(args, "sde_seed", None) is None
                                                         else {"sample_base": split_index[group[0]]}))
        sync()
        dur = time.time() - start
        nfr = len(group) * args.num_rollouts * args.num_frames
        total_frames, total_s = total_frames + nfr, total_s + dur
        print(f"{','.join(group)}: {nfr / dur:.1f} frames/s ({dur:.3f} s, batch {len(group)})")
        # a device tensor is formatted on the device (pdb.py); the host copy is made only for what needs one
        host = all_atom14.cpu().numpy() if args.npy or not all_atom14.is_cuda else None
        for i, n in enumerate(group):
            aat = np.array([restype_order[c] for c in seqres[n]])
            written = all_atom14[i] if all_atom14.is_cuda else host[i]
            if getattr(args, "superpose", False):
                from .ensemble import superpose_on_first
                written = superpose_on_first(all_atom14[i], aat)
            atom14_to_pdb(written, aat, os.path.join(args.out_dir, f"{n}.pdb"))
            if getattr(args, "xtc", False):
                write_xtc(os.path.join(args.out_dir, f"{n}.pdb"), os.path.join(args.out_dir, f"{n}.xtc"))
            if args.npy:
                np.save(os.path.join(args.out_dir, f"{n}.npy"), written.cpu().numpy() if getattr(args, "superpose", False) else host[i])
            if getattr(args, "analyze", False):
                from .analyze_peptide_sim import analyze_one, msm_options
                sync()
                start = time.time()
                with_msm = getattr(args, "msm", False)
                analysis[n] = analyze_one(n, all_atom14[i], arrs[n], aat, tica=getattr(args, "tica", False) or with_msm,
                                          tica_lag=getattr(args, "tica_lag", 1000), msm=msm_options(args) if with_msm else None)
                if getattr(args, "ensemble", False):
                    from .ensemble import analyze_ensemble
                    from .analyze_ensembles import sasa_options
                    analysis[n]["ensemble"] = analyze_ensemble(all_atom14[i], arrs[n], aat, **sasa_options(args))
                sync()
                analysis_s += time.time() - start
    job_s = max_over_ranks(total_s, dist)
    job_frames = sum_over_ranks(total_frames, dist)
    if dist is not None:
        dist.barrier()
    if getattr(args, "analyze", False):
        import pickle
        with open(os.path.join(args.out_dir, "analysis.pkl" if world == 1 else f"analysis.rank{rank}.pkl"), "wb") as f:
            pickle.dump(analysis, f)
        print(f"analysis: {len(analysis)} peptides in {analysis_s:.3f} s (not part of the frames/s above)")
    if job_s > 0:
        print(f"rank {rank}/{world}: {len(names)} peptides, {total_frames} frames in {total_s:.3f} s; "
              f"job: {job_frames / job_s:.1f} frames/s")
    return {"names": names, "frames": total_frames, "seconds": total_s, "job_frames": int(job_frames),
            "job_seconds": job_s}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--sim_ckpt", type=str, default=None)
    p.add_argument("--data_dir", type=str, required=True)
    p.add_argument("--suffix", type=str, default="")
    p.add_argument("--pdb_id", nargs="*", default=[])
    p.add_argument("--num_frames", type=int, default=1000)
    p.add_argument("--num_rollouts", type=int, default=100)
    p.add_argument("--no_frames", action="store_true")
    p.add_argument("--tps", action="store_true")
    p.add_argument("--xtc", action="store_true")
    p.add_argument("--out_dir", type=str, default=".")
    p.add_argument("--split", type=str, default="splits/4AA_test.csv")
    add_solver_arguments(p, per="block")
    p.add_argument("--batch", type=int, default=1, help="peptides of equal length per inference() call")
    p.add_argument("--chunk_idx", type=int, default=0)
    p.add_argument("--n_chunks", type=int, default=1)
    p.add_argument("--per_block", action="store_true",
                   help="one inference() call per block from Python instead of the multi-block device rollout")
    p.add_argument("--precision", choices=["bf16", "fp32"], default="bf16",
                   help="bf16 MFMA operands (default) or the fp32-operand tolerance mode (~10x slower)")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic weights instead of --sim_ckpt")
    p.add_argument("--npy", action="store_true", help="also save the sampled atom14 array as .npy")
    p.add_argument("--analyze", action="store_true",
                   help="torsion JSDs and decorrelation curves against the conditioning trajectory -> {out_dir}/analysis.pkl")
    p.add_argument("--tica", action="store_true",
                   help="with --analyze: also the tICA entries (TICA-0 / TICA-0,1 JSDs, 'tica' curves, tica_model); a peptide whose "
                        "MD trajectory is too short for the lag is named on stderr and keeps its torsion entries")
    p.add_argument("--tica_lag", type=int, default=1000, help="the tICA lag in frames of the MD trajectory (reference: 1000)")
    p.add_argument("--msm", action="store_true",
                   help="with --analyze: also the k-means / MSM / PCCA+ entries (implies --tica); a peptide whose MSM is refused is "
                        "named on stderr and keeps its other entries")
    p.add_argument("--msm_k", type=int, default=100, help="k-means microstates (reference: 100)")
    p.add_argument("--msm_states", type=int, default=10, help="PCCA+ metastable states (reference: 10)")
    p.add_argument("--md_msm_lag", type=int, default=1000, help="the MD trajectory's MSM lag in frames (reference: 1000)")
    p.add_argument("--msm_lag", type=int, default=10, help="the sampled trajectory's MSM lag in frames (reference: 10)")
    p.add_argument("--kmeans_seed", type=int, default=137, help="seed of the k-means++ uniforms (reference: fixed_seed=137)")
    p.add_argument("--no_traj_msm", action="store_true", help="skip the sampled trajectory's own MSM")
    p.add_argument("--ensemble", action="store_true",
                   help="with --analyze: also mdgen_amd.ensemble.analyze_ensemble's dict (RMSF, pairwise RMSD, Gaussian W2, contacts, "
                        "PCA) under analysis[name]['ensemble']; with --sasa also the solvent-accessible-surface entries")
    from .analyze_ensembles import add_sasa_arguments
    add_sasa_arguments(p)
    p.add_argument("--superpose", action="store_true",
                   help="superpose each written trajectory (PDB and --npy) on its own first frame over its existing atoms, on the "
                        "device (the reference's traj.superpose(traj))")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    solver_kwargs(args)   # (the command line's solver refusals, before anything is loaded)
    if args.no_frames or args.tps:
        raise SystemExit("--no_frames / --tps are outside this build's scope (see DESIGN.md)")
    import pandas as pd
    from .config import ModelConfig
    from .synthetic import synth_state_dict
    from .wrapper import NewMDGenWrapper
    rank, world, local_rank = dist_env()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    dist = None
    if world > 1:   # one process per GPU (torch.distributed.run); RCCL is used for the barrier and the timing only
        import torch.distributed as dist_
        if not dist_.is_initialized():
            dist_.init_process_group("nccl", device_id=device)
        dist = dist_
    df = pd.read_csv(args.split, index_col="name")
    names_seqres = {str(n): df.seqres[n] for n in df.index}
    if args.synthetic:
        # (the position table of the seeded model covers the split's longest sequence: 4 for the tetrapeptide splits, as before)
        cfg = ModelConfig.forward_sim(num_frames=args.num_frames, crop=max([4] + [len(s) for s in names_seqres.values()]))
        model = NewMDGenWrapper(cfg, device=device, precision=args.precision)
        model.model.load_state_dict(synth_state_dict(cfg, 0))
    else:
        if not args.sim_ckpt:
            raise SystemExit("--sim_ckpt is required (or --synthetic)")
        model = NewMDGenWrapper.load_from_checkpoint(args.sim_ckpt, device=device, precision=args.precision)
    return run(args, model, device, names_seqres, rank, world, sync=torch.cuda.synchronize, dist=dist)


if __name__ == "__main__":
    with torch.no_grad():
        main()
