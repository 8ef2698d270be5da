"""Analysis driver with the options of the reference's `scripts/analyze_peptide_sim.py`:

  --pdbdir DIR       the sampled trajectories: `{name}.npy` (what `sim_inference --npy` writes) when present, else `{name}.pdb`,
                     this project's multi-model PDB, read by `mdgen_amd.pdb.pdb_to_atom14`;
  --data_dir DIR     the MD trajectories `{data_dir}/{name}{suffix}.npy`, atom14 arrays (in place of the reference's --mddir of
                     XTC files);  --suffix;  --split CSV  the sequences (columns name, seqres);
  --pdb_id ...       the peptides (default: every name of the split with a trajectory in --pdbdir);
  --truncate N       only the first N sampled frames;  --no_decorr  skip the decorrelation curves;
  --save / --save_name   pickle {name: result} to `{pdbdir}/{save_name}`;
  --tica [--tica_lag N]   also the tICA entries (`analyze(tica=True)`: JSD "TICA-0" / "TICA-0,1", the "tica" decorrelation
                     curves, "tica_model"), fitted on the MD trajectory at lag N (default 1000).  A peptide whose MD trajectory
                     is too short for the lag (or whose covariance has rank < 2) is named on stderr and gets the other entries;
  --msm              also the k-means / MSM / PCCA+ entries (`analyze(msm=True)`, which implies --tica): "kmeans", "msm", "pcca",
                     "cmsm", the metastable-state occupancies, the coarse transition matrix and stationary distributions, by this
                     project's restatement of the estimators (mdgen_amd/msm.py; agreement with pyemma is unverified).
                     --msm_k N (100) microstates, --msm_states N (10) metastable states, --md_msm_lag N (1000) the MD MSM's lag,
                     --msm_lag N (10) the sampled trajectory's, --kmeans_seed N (137);  --no_traj_msm skips the sampled
                     trajectory's own MSM.  A peptide whose MSM is refused (a microstate outside the connected set, too few
                     frames) is named on stderr and gets the other entries;
  --no_msm           without the MSM entries.  One of --msm and --no_msm is REQUIRED (they exclude each other): with neither the
                     command is refused before anything is read (exit status 2), so that a pipeline that expects the reference's
                     pyemma objects does not find out afterwards.

Per peptide the result is `mdgen_amd.analysis.analyze`'s dict: "features", "JSD", "our_decorrelation", "md_decorrelation"
(and "tica_model" with --tica, the MSM entries with --msm).
No plots (--plot does not exist), no XTC files."""
from __future__ import annotations

import argparse
import csv
import os
import pickle
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--pdbdir", type=str, required=True)
    p.add_argument("--data_dir", type=str, default="share/4AA_sims")
    p.add_argument("--suffix", type=str, default="")
    p.add_argument("--split", type=str, default="splits/4AA_test.csv")
    p.add_argument("--pdb_id", nargs="*", default=[])
    p.add_argument("--truncate", type=int, default=None)
    p.add_argument("--no_decorr", action="store_true")
    p.add_argument("--save", action="store_true")
    p.add_argument("--save_name", type=str, default="out.pkl")
    which = p.add_mutually_exclusive_group()
    which.add_argument("--no_msm", action="store_true")
    which.add_argument("--msm", action="store_true")
    p.add_argument("--no_traj_msm", action="store_true")
    p.add_argument("--msm_k", type=int, default=100)
    p.add_argument("--msm_states", type=int, default=10)
    p.add_argument("--md_msm_lag", type=int, default=1000)
    p.add_argument("--msm_lag", type=int, default=10)
    p.add_argument("--kmeans_seed", type=int, default=137)
    p.add_argument("--tica", action="store_true")
    p.add_argument("--tica_lag", type=int, default=1000)
    return p


def require_no_msm(args):
    """The policy of `sim_inference.require_xtc_writer`: what cannot be delivered is refused before any work is done."""
    if not args.no_msm and not args.msm:
        print("error: the tICA / MSM analysis needs pyemma (the reference's dependency for its estimators), which this project "
              "does not use; run with --no_msm for the torsion JSDs and the decorrelation curves", file=sys.stderr)
        raise SystemExit(2)


def read_split(path):
    with open(path, newline="") as f:
        return {row["name"]: row["seqres"] for row in csv.DictReader(f)}


def trajectory_path(pdbdir, name):
    for ext in (".npy", ".pdb"):
        p = os.path.join(pdbdir, name + ext)
        if os.path.exists(p):
            return p
    raise SystemExit(f"error: no sampled trajectory of {name}: neither {os.path.join(pdbdir, name)}.npy nor .pdb exists")


def load_trajectory(path, aatype):
    from .pdb import pdb_to_atom14
    return np.load(path, mmap_mode="r") if path.endswith(".npy") else pdb_to_atom14(path, aatype)


def msm_options(args) -> dict:
    """`analyze`'s MSM keywords from the parsed options."""
    return dict(msm=True, msm_k=args.msm_k, msm_states=args.msm_states, md_msm_lag=args.md_msm_lag, msm_lag=args.msm_lag,
                traj_msm=not args.no_traj_msm, kmeans_seed=args.kmeans_seed)


def analyze_one(name, traj, ref, aatype, tica=False, tica_lag=1000, msm=None, **kw):
    """`analyze`; a peptide whose tICA is refused (MD trajectory too short for the lag, rank < 2, no torsions) is named on stderr
    and analysed without the tICA entries.  `msm`: `msm_options`' dict or None; a peptide whose MSM is refused is named on stderr
    and analysed without the MSM entries."""
    from .analysis import analyze
    if msm:
        try:
            return analyze(traj, ref, aatype, tica=True, tica_lag=tica_lag, name=name, **msm, **kw)
        except ValueError as e:
            print(f"{name}: no MSM entries: {e}", file=sys.stderr)
    if tica:
        try:
            return analyze(traj, ref, aatype, tica=True, tica_lag=tica_lag, **kw)
        except ValueError as e:
            print(f"{name}: no tICA entries: {e}", file=sys.stderr)
    return analyze(traj, ref, aatype, **kw)


def main(argv=None):
    args = build_parser().parse_args(argv)
    require_no_msm(args)
    seqres = read_split(args.split)
    if args.pdb_id:
        names = list(args.pdb_id)
        unknown = [n for n in names if n not in seqres]
        if unknown:
            raise SystemExit(f"error: {unknown} not in {args.split}")
    else:
        have = {os.path.splitext(f)[0] for f in os.listdir(args.pdbdir) if f.endswith((".npy", ".pdb"))}
        names = [n for n in seqres if n in have]
    paths = {n: trajectory_path(args.pdbdir, n) for n in names}   # (every missing file is found before the first is analysed)
    refs = {n: f"{args.data_dir}/{n}{args.suffix}.npy" for n in names}
    for n, p in refs.items():
        if not os.path.exists(p):
            raise SystemExit(f"error: no MD trajectory of {n}: {p} does not exist")
    print("number of trajectories", len(names))
    import torch
    from .geometry import restype_order
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    out = {}
    for n in names:
        aat = np.array([restype_order[c] for c in seqres[n]])
        traj = load_trajectory(paths[n], aat)
        if args.truncate:
            traj = traj[:args.truncate]
        traj = torch.from_numpy(np.array(traj, np.float32)).to(device)   # (a copy: the memory map is read-only)
        out[n] = analyze_one(n, traj, np.load(refs[n], mmap_mode="r"), aat, decorr=not args.no_decorr, tica=args.tica or args.msm,
                             tica_lag=args.tica_lag, msm=msm_options(args) if args.msm else None)
        jsd = out[n]["JSD"]
        print(f"{n}: {len(out[n]['features'])} torsions, mean JSD {np.mean(list(jsd.values())) if jsd else float('nan'):.4f}")
    if args.save:
        with open(os.path.join(args.pdbdir, args.save_name), "wb") as f:
            f.write(pickle.dumps(out))
    return out


if __name__ == "__main__":
    main()
