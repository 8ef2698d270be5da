"""Ensemble analysis driver for proteins (the ATLAS models): `mdgen_amd.ensemble.analyze_ensemble` of every protein of a split.

  --pdbdir DIR       the sampled trajectories: `{name}.npy` (what `sim_inference --npy` writes) when present, else `{name}.pdb`,
                     this project's multi-model PDB, read by `mdgen_amd.pdb.pdb_to_atom14`;
  --data_dir DIR     the MD trajectories, atom14 arrays `{data_dir}/{name}{suffix}.npy`;  --split CSV  (columns name, seqres);
  --suffix S         with --ref_suffixes absent, the one MD replica to compare with (default "");
  --ref_suffixes ... the replicas concatenated as the MD ensemble, e.g. `_R1 _R2 _R3`; its first frame is the reference structure;
  --pdb_id ...       the proteins (default: every name of the split);
  --fit heavy|ca     superpose over the existing heavy atoms (default) or the C-alphas;  --cutoff A  contact cutoff (8);
  --no_pca           without the PCA entries;  --save  pickle {name: result} to `{pdbdir}/ensemble.pkl`;
  --sasa             with the solvent-accessible-surface entries (residue areas, exposure probabilities, exposed-residue Jaccard,
                     exposure mutual information and its Spearman correlation), under --probe A (2.8), --sasa_points N (960),
                     --sasa_threshold A^2 (2.0) and --sasa_atoms sidechain|all.

A protein whose files are missing or whose shapes disagree is named on stderr and skipped.  The result is a dict of plain NumPy
arrays and floats per protein (it loads without this package).  No plots, no XTC files."""
from __future__ import annotations

import argparse
import os
import pickle
import sys

import numpy as np

from .analyze_peptide_sim import load_trajectory, read_split


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--pdbdir", type=str, required=True)
    p.add_argument("--data_dir", type=str, required=True)
    p.add_argument("--split", type=str, required=True)
    p.add_argument("--suffix", type=str, default="")
    p.add_argument("--ref_suffixes", nargs="*", default=None)
    p.add_argument("--pdb_id", nargs="*", default=[])
    p.add_argument("--fit", choices=["heavy", "ca"], default="heavy")
    p.add_argument("--cutoff", type=float, default=8.0)
    p.add_argument("--no_pca", action="store_true")
    p.add_argument("--save", action="store_true")
    add_sasa_arguments(p)
    return p


def add_sasa_arguments(p):
    """--sasa and its options, for every command line that calls `analyze_ensemble`."""
    p.add_argument("--sasa", action="store_true", help="also the solvent-accessible-surface entries of analyze_ensemble")
    p.add_argument("--probe", type=float, default=2.8, help="probe radius in Angstrom")
    p.add_argument("--sasa_points", type=int, default=960, help="sphere points per atom")
    p.add_argument("--sasa_threshold", type=float, default=2.0, help="a residue is exposed above this area (A^2)")
    p.add_argument("--sasa_atoms", choices=["sidechain", "all"], default="sidechain")


def sasa_options(args) -> dict:
    """The keyword arguments `analyze_ensemble` takes for --sasa: none without it.  Bad values end the run before any file is read."""
    if not getattr(args, "sasa", False):
        return {}
    if not (np.isfinite(args.probe) and 0 <= args.probe <= 16):
        raise SystemExit(f"error: --probe must be in 0 .. 16, got {args.probe}")
    if not 1 <= args.sasa_points <= 4096:
        raise SystemExit(f"error: --sasa_points must be in 1 .. 4096, got {args.sasa_points}")
    if not np.isfinite(args.sasa_threshold):
        raise SystemExit(f"error: --sasa_threshold must be finite, got {args.sasa_threshold}")
    return dict(sasa=True, probe=args.probe, n_points=args.sasa_points, sasa_threshold=args.sasa_threshold, sasa_atoms=args.sasa_atoms)


def load_protein(args, name, seq):
    """(traj, ref, aatype) of one protein, or a string saying why it is skipped."""
    from .geometry import restype_order
    unknown = sorted(set(seq) - set(restype_order))
    if unknown:
        return f"residues {unknown} are not amino-acid letters"
    aat = np.array([restype_order[c] for c in seq])
    path = next((os.path.join(args.pdbdir, name + ext) for ext in (".npy", ".pdb")
                 if os.path.exists(os.path.join(args.pdbdir, name + ext))), None)
    if path is None:
        return f"neither {os.path.join(args.pdbdir, name)}.npy nor .pdb exists"
    suffixes = args.ref_suffixes if args.ref_suffixes else [args.suffix]
    refs = [f"{args.data_dir}/{name}{s}.npy" for s in suffixes]
    missing = [r for r in refs if not os.path.exists(r)]
    if missing:
        return f"no MD trajectory {', '.join(missing)}"
    try:
        traj = np.asarray(load_trajectory(path, aat))
    except (ValueError, KeyError, IndexError) as e:
        return f"{path} cannot be read as {len(aat)} residues: {e}"
    want = (len(aat), 14, 3)
    if traj.ndim != 4 or traj.shape[1:] != want or traj.shape[0] < 1:
        return f"{path} has shape {traj.shape}, the sequence needs [T, {len(aat)}, 14, 3]"
    parts = [np.load(r, mmap_mode="r") for r in refs]
    for r, a in zip(refs, parts):
        if a.ndim != 4 or a.shape[1:] != want or a.shape[0] < 1:
            return f"{r} has shape {a.shape}, the sequence needs [F, {len(aat)}, 14, 3]"
    ref = parts[0] if len(parts) == 1 else np.concatenate(parts, 0)
    return traj, ref, aat


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not (np.isfinite(args.cutoff) and args.cutoff > 0):
        raise SystemExit(f"error: --cutoff must be positive, got {args.cutoff}")
    sasa = sasa_options(args)
    seqres = read_split(args.split)
    names = list(args.pdb_id) if args.pdb_id else list(seqres)
    unknown = [n for n in names if n not in seqres]
    if unknown:
        raise SystemExit(f"error: {unknown} not in {args.split}")
    from . import ensemble
    out = {}
    for n in names:
        got = load_protein(args, n, seqres[n])
        if isinstance(got, str):
            print(f"{n}: skipped: {got}", file=sys.stderr)
            continue
        traj, ref, aat = got
        out[n] = ensemble.analyze_ensemble(traj, ref, aat, fit=args.fit, cutoff=args.cutoff, pca=not args.no_pca, **sasa)
        r = out[n]
        print(f"{n}: {traj.shape[0]} frames against {ref.shape[0]}: RMSF r {r['rmsf_pearson']:.3f}, pairwise RMSD "
              f"{r['mean_pairwise_rmsd']:.2f} (MD {r['ref_mean_pairwise_rmsd']:.2f}), RMWD {r['emd_total']:.2f}, weak contacts J "
              f"{r['weak_contacts_jaccard']:.2f}, transient {r['transient_contacts_jaccard']:.2f}"
              + (f", exposed residues J {r['exposed_residue_jaccard']:.2f}, exposure MI rho {r['exposed_mi_spearman']:.2f}" if sasa else ""))
    print(f"{len(out)} of {len(names)} proteins analysed")
    if args.save:
        with open(os.path.join(args.pdbdir, "ensemble.pkl"), "wb") as f:
            pickle.dump(out, f)
    return out


if __name__ == "__main__":
    main()
