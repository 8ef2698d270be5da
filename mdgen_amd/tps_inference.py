"""Transition-path (two-sided conditioning) batch layout, mirroring the reference's
`tps_inference.get_sample` (tps_inference.py:43-80): the start frame's torsions / translations / rotations are
expanded over `num_frames` and frame -1 is replaced by the end frame's; `NewMDGenWrapper.prep_batch` then marks
frames 0 and -1 as conditioning (wrapper.py:341-342) and the model runs its IPA stack on both frame sets.

The end states.  With `--msm` they are chosen as the reference chooses them (tps_inference.py:82-118): a Markov-state model of the
MD trajectory `{data_dir}/{name}{suffix}.npy` -- torsions -> tICA -> k-means -> MSM -> PCCA+ -> coarse MSM, on the device
(mdgen_amd/analysis.py `md_msm`; the k x k estimators are mdgen_amd/msm.py's restatement of pyemma's, agreement unverified) --
gives the pair of metastable states of least flux (`msm.least_flux_pair`), and every path draws its own start and end frame from
the MD frames of those states (`msm.tps_endpoints`, seeded by --tps_seed and the peptide's index in the split: reproducible, the
same on one rank or many; statistically the reference's choice, not draw for draw -- the reference draws from NumPy's unseeded
global state).  The model is written to `{out_dir}/{name}_metadata.pkl` under the reference's keys (msm, cmsm, pcca, kmeans, tica,
ref_kmeans) as plain dicts and arrays, and read back from there when it exists; `{name}_metadata.json` lists every path's
{name, start_idx, end_idx, start_state, end_state, path}, and a peptide that has one is skipped -- both as the reference does.
`python -m mdgen_amd.analyze_peptide_tps` scores the paths from those two files.
Without `--msm` the two MD frames are given explicitly (--start_frame, --end_frame) and every path shares them.

The geometry (atom14 -> frames, torsions) runs on the device through the same glue kernel the forward-simulation rollout uses
(`mdgen_atom14_to_cond`).  No XTC files.  `--superpose` (off by default) superposes every written path (PDB and --npy) on its own
first frame over its existing atoms, unweighted, on the device before it is formatted (`mdgen_ens_superpose`)."""
from __future__ import annotations

import numpy as np
import torch

from .solver import add_solver_arguments, solver_kwargs


def get_sample(start_arr, end_arr, seqres_str: str, num_frames: int, device="cuda"):
    """start_arr / end_arr: atom14 coordinates [1, L, 14, 3] (or [L, 14, 3]) of the two end states, Angstrom.
    Returns the batch dict of tps_inference.py:68-79 with a leading batch dimension of 1 (what the reference's
    DataLoader collation adds): torsions (1,T,L,7,2), torsion_mask (1,L,7), trans (1,T,L,3), rots (1,T,L,3,3),
    seqres (1,L), mask (1,L)."""
    from .geometry import atom14_to_cond, restype_order

    def frame(a):
        a = np.asarray(a, dtype=np.float32)
        if a.ndim == 3:
            a = a[None]
        return torch.from_numpy(np.copy(a[0:1])).to(device)

    seqres = torch.tensor([restype_order[c] for c in seqres_str], device=device)[None]
    s = atom14_to_cond(frame(start_arr), seqres)
    e = atom14_to_cond(frame(end_arr), seqres)
    T = int(num_frames)

    def traj(key):
        x = s[key][:, None].expand(-1, T, *s[key].shape[1:]).clone()
        x[:, -1] = e[key]
        return x

    L_ = seqres.shape[1]
    return {"torsions": traj("torsions"), "torsion_mask": s["torsion_mask"], "trans": traj("trans"),
            "rots": traj("rots"), "seqres": seqres, "mask": torch.ones(1, L_, device=device)}


def collate(samples):
    """Stack `get_sample` dicts along the batch dimension (the reference uses a DataLoader for this, :127)."""
    return {k: torch.cat([s[k] for s in samples], 0) for k in samples[0]}


def build_parser():
    """Arguments of the reference's driver (tps_inference.py:6-18) -- its `--mddir` of XTC files is `--data_dir`'s atom14 arrays --
    plus `--msm` with the estimator options of analyze_peptide_sim (names and defaults) and `--tps_seed`, the two explicit MD frame
    indices used without it, `--npy`, `--num_steps` and `--synthetic`."""
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument("--sim_ckpt", type=str, default=None)
    p.add_argument("--data_dir", type=str, default="share/4AA_data")
    p.add_argument("--suffix", type=str, default="")
    p.add_argument("--pdb_id", nargs="*", default=[])
    p.add_argument("--num_frames", type=int, default=1000)
    p.add_argument("--num_batches", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=10)
    p.add_argument("--out_dir", type=str, default=".")
    p.add_argument("--split", type=str, default="splits/4AA_test.csv")
    p.add_argument("--chunk_idx", type=int, default=0)
    p.add_argument("--n_chunks", type=int, default=1)
    p.add_argument("--start_frame", type=int, default=0, help="MD frame of {name}.npy used as the start state")
    p.add_argument("--end_frame", type=int, default=-1, help="MD frame of {name}.npy used as the end state")
    p.add_argument("--msm", action="store_true", help="choose start / end states and frames from an MSM of the MD trajectory")
    p.add_argument("--tica_lag", type=int, default=1000)
    p.add_argument("--msm_k", type=int, default=100)
    p.add_argument("--msm_states", type=int, default=10)
    p.add_argument("--md_msm_lag", type=int, default=1000)
    p.add_argument("--kmeans_seed", type=int, default=137)
    p.add_argument("--tps_seed", type=int, default=137, help="seed of the start / end frame draws (--msm)")
    p.add_argument("--npy", action="store_true", help="also write every path as {name}_{idx}.npy")
    add_solver_arguments(p, per="batch of paths")
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--superpose", action="store_true", help="superpose each written trajectory (PDB and --npy) on its own first frame over its existing atoms, on the device "
                        "(the reference's traj.superpose(traj))")
    return p


METADATA_KEYS = ("msm", "cmsm", "tica", "pcca", "kmeans", "ref_kmeans")   # the reference's pickle (tps_inference.py:101-108)


def build_metadata(ref_atom14, aatype, tica_lag=1000, msm_k=100, msm_states=10, md_msm_lag=1000, kmeans_seed=137, device="cuda"):
    """The reference's `{name}_metadata.pkl` from the MD trajectory (atom14 [F, L, 14, 3]): featurize -> `tica_fit` -> projection
    at the model's `dim` -> `analysis.md_msm` (k-means, MSM, PCCA+, coarse MSM).  Plain dicts and arrays under METADATA_KEYS;
    "tica" is `TicaModel.as_dict()`, "ref_kmeans" the MD trajectory's microstates, int32 [F].  ValueError as `analysis.analyze`."""
    from . import analysis as A
    ref = A._device_f32(ref_atom14, device)
    a_ref = A.featurize(ref, aatype)
    model = A.tica_fit(a_ref, tica_lag)
    entries, d_ref = A.md_msm(A.tica_transform(model, a_ref, model.dim), msm_k, msm_states, md_msm_lag, kmeans_seed)
    entries.update(tica=model.as_dict(), ref_kmeans=d_ref.cpu().numpy().astype(np.int32))
    return {key: entries[key] for key in METADATA_KEYS}


def load_or_build_metadata(path, arr, aatype, args, device):
    import os
    import pickle
    if os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    meta = build_metadata(arr, aatype, args.tica_lag, args.msm_k, args.msm_states, args.md_msm_lag, args.kmeans_seed, device)
    with open(path, "wb") as f:
        pickle.dump(meta, f)
    return meta


def run(args, model, device, names_seqres, rank=0, world=1):
    """tps_inference.py:118-168 (`do` + `main`): for every peptide of this process's chunk / rank shard,
    `num_batches` batches of `batch_size` transition paths between the two end states -> `{name}_{idx}.pdb` (with --npy also
    `.npy`).  With --msm the end states are the MSM's and the two metadata files are written (module docstring); a peptide whose
    MSM is refused, or whose MD trajectory has no frame in a chosen state, is named on stderr and skipped."""
    import json
    import os
    import sys
    from .geometry import restype_order
    from .pdb import atom14_to_pdb
    from .sim_inference import select_names
    kw = solver_kwargs(args)
    names = select_names(list(names_seqres), args.pdb_id, args.chunk_idx, args.n_chunks, rank, world)
    os.makedirs(args.out_dir, exist_ok=True)
    done = []
    split_index = {n: i for i, n in enumerate(names_seqres)}
    per_peptide = args.num_batches * args.batch_size
    for name in names:
        meta_json = os.path.join(args.out_dir, f"{name}_metadata.json")
        if args.msm and os.path.exists(meta_json):     # (the reference's resume rule, tps_inference.py:84-85)
            continue
        arr = np.lib.format.open_memmap(f"{args.data_dir}/{name}{args.suffix}.npy", "r")
        seq = names_seqres[name]
        aat = np.array([restype_order[c] for c in seq])
        if args.msm:
            from . import msm as M
            try:
                pkl = load_or_build_metadata(os.path.join(args.out_dir, f"{name}_metadata.pkl"), arr, aat, args, device)
                start_state, end_state, start_idx, end_idx = M.tps_endpoints(
                    pkl["cmsm"], pkl["pcca"]["metastable_assignments"], pkl["ref_kmeans"], per_peptide, args.tps_seed,
                    split_index[name])
            except ValueError as e:
                print(f"{name}: skipped: {e}", file=sys.stderr)
                continue
            records = []
        else:
            batch = collate([get_sample(arr[args.start_frame], arr[args.end_frame], seq, args.num_frames, device)] * args.batch_size)
        for i in range(args.num_batches):
            if args.msm:       # every path has its own end frames
                which = range(i * args.batch_size, (i + 1) * args.batch_size)
                batch = collate([get_sample(arr[int(start_idx[p])], arr[int(end_idx[p])], seq, args.num_frames, device) for p in which])
            if "rng_seed" in kw:   # --sde_seed: path idx of the peptide at index p of the split draws at (sample idx, block p),
                kw.update(rng_sample_base=i * args.batch_size, rng_block_base=split_index[name])   # whichever rank samples it
            atom14s, _ = model.inference(batch, **kw)
            if kw.get("sampling_method") == "dopri5":
                st = model.last_stats
                print(f"{name} batch {i}: dopri5 {st['nfe']} network evaluations ({st['accepted']} accepted, "
                      f"{st['rejected']} rejected steps)")
            if getattr(args, "superpose", False):
                from .ensemble import superpose_on_first
                atom14s = torch.stack([superpose_on_first(a, aat) for a in atom14s])
            paths = atom14s if atom14s.is_cuda else atom14s.cpu().numpy()   # (a device tensor is formatted on the device, pdb.py)
            for j in range(args.batch_size):
                idx = i * args.batch_size + j
                path = os.path.join(args.out_dir, f"{name}_{idx}.pdb")
                atom14_to_pdb(paths[j], aat, path)
                if args.npy:
                    np.save(os.path.join(args.out_dir, f"{name}_{idx}.npy"), paths[j].cpu().numpy() if atom14s.is_cuda else paths[j])
                if args.msm:
                    records.append({"name": name, "start_idx": int(start_idx[idx]), "end_idx": int(end_idx[idx]),
                                    "start_state": int(start_state), "end_state": int(end_state), "path": path})
        if args.msm:
            with open(meta_json, "w") as f:
                json.dump(records, f)
        done.append(name)
    return {"names": done, "paths": len(done) * args.num_batches * args.batch_size}


def main(argv=None):
    import pandas as pd
    from .config import ModelConfig
    from .sim_inference import dist_env
    from .synthetic import synth_state_dict
    from .wrapper import NewMDGenWrapper
    args = build_parser().parse_args(argv)
    solver_kwargs(args)   # (the command line's solver refusals, before anything is loaded)
    rank, world, local_rank = dist_env()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    if args.synthetic:
        cfg = ModelConfig.tps(num_frames=args.num_frames)
        model = NewMDGenWrapper(cfg, device=device)
        model.model.load_state_dict(synth_state_dict(cfg, 0))
    else:
        if not args.sim_ckpt:
            raise SystemExit("--sim_ckpt is required (or --synthetic)")
        model = NewMDGenWrapper.load_from_checkpoint(args.sim_ckpt, device=device)
    df = pd.read_csv(args.split, index_col="name")
    return run(args, model, device, {str(n): df.seqres[n] for n in df.index}, rank, world)


if __name__ == "__main__":
    with torch.no_grad():
        main()
