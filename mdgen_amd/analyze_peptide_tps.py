"""Transition-path analysis with the options of the reference's `scripts/analyze_peptide_tps.py`, from what
`tps_inference --msm` wrote:

  --pdbdir DIR       `{name}_metadata.pkl` (the MD trajectory's tICA model, k-means centres, MSM, PCCA+ and coarse MSM),
                     `{name}_metadata.json` (one record per path) and the paths `{name}_{i}.npy` when present, else `{name}_{i}.pdb`;
  --outdir DIR       `{name}.pkl` per peptide;  --save / --save_name  also the dict over peptides, `{outdir}/{save_name}`;
  --repdir DIR       the replica MD trajectories `{repdir}/{name}{suffix}.npy`, atom14 arrays (in place of the reference's XTC
                     files); a peptide without one is named on stderr and gets no `rep` keys;  --suffix;
  --split CSV        the sequences (columns name, seqres);  --pdb_id ...  the peptides (default: every name of the split with a
                     `_metadata.json` in --pdbdir);
  --stride N (10)    a path's frames 0, N, 2N, ... and its last frame again are kept: the reference's `[:, ::10]` plus `[:, -1:]`;
  --n_samples (1000), --seed (137)   the sampled reference and replica paths (`analysis.tp_sample`: stream 0 the reference's,
                     stream 1 + i replica length i's);
  --rep_lens / --rep_names   the replica prefixes and their key prefixes (default: the reference's seven, 999999 .. 20000 frames,
                     "100ns" .. "2ns").

Per peptide the result is the metadata pickle's entries plus the reference's keys -- gen_prob, gen_valid_prob, gen_valid_rate,
gen_JSD and, per replica length, {rep_name}_rep_{prob, valid_prob, valid_rate, JSD} and the identical _repcheat_ four -- plus
ref_stateprobs, gen_stateprobs, traj_len, and the exact expectations the sampled figures estimate (`msm.bridge_exact`):
ref_stateprobs_exact, gen_JSD_exact, {rep_name}_rep_{prob, valid_prob, valid_rate, JSD}_exact.

What differs from the reference, on purpose.  The tICA model is the pickle's: the MD trajectory is not read at all.  Sampled paths
are statistically the reference's, not draw for draw (another generator).  The likelihood is the reference's expression
(`msm.tp_likelihood`).  A state outside the coarse MSM's active set is scored as the active state of largest pi -- by its matrix
INDEX argmax(pi); the reference's fallback is active_set[argmax pi], a state number used as an index; the two agree whenever all
states are active, as do state numbers and matrix indices everywhere else.  No --plot, no --num_workers, no TPT fluxes.  Agreement
of the estimators with pyemma is unverified (mdgen_amd/msm.py)."""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys

import numpy as np

from .analyze_peptide_sim import read_split

REP_LENS = [999999, 500000, 300000, 200000, 100000, 50000, 20000]      # analyze_peptide_tps.py:87-88
REP_NAMES = ["100ns", "50ns", "30ns", "20ns", "10ns", "5ns", "2ns"]
METRICS = ("prob", "valid_prob", "valid_rate", "JSD")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--pdbdir", type=str, required=True)
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--repdir", type=str, default="share/4AA_sims_replica")
    p.add_argument("--suffix", type=str, default="")
    p.add_argument("--split", type=str, default="splits/4AA_test.csv")
    p.add_argument("--pdb_id", nargs="*", default=[])
    p.add_argument("--save", action="store_true")
    p.add_argument("--save_name", type=str, default="out.pkl")
    p.add_argument("--stride", type=int, default=10)
    p.add_argument("--n_samples", type=int, default=1000)
    p.add_argument("--seed", type=int, default=137)
    p.add_argument("--rep_lens", type=int, nargs="+", default=list(REP_LENS))
    p.add_argument("--rep_names", type=str, nargs="+", default=list(REP_NAMES))
    return p


def load_metadata(pdbdir, name):
    """(the pickle's dict, the json's list of path records); a missing file is a named error."""
    paths = [os.path.join(pdbdir, f"{name}_metadata.{ext}") for ext in ("json", "pkl")]
    for p in paths:
        if not os.path.exists(p):
            raise SystemExit(f"error: no transition-path metadata of {name}: {p} does not exist (tps_inference --msm writes it)")
    with open(paths[0]) as f:
        records = json.load(f)
    with open(paths[1], "rb") as f:
        pkl = pickle.load(f)
    if not records:
        raise SystemExit(f"error: {paths[0]} lists no path")
    return pkl, records


def strided_frames(F, stride):
    """Frames 0, stride, 2 stride, ... of F and the last frame again: `[:, ::stride]` plus `[:, -1:]`."""
    return list(range(0, int(F), int(stride))) + [int(F) - 1]


def load_paths(pdbdir, name, n_paths, aatype, stride):
    """(atom14 fp32 [P, N, L, 14, 3], F): the kept frames of every path, `.npy` before `.pdb`, gathered before anything is
    featurized.  Every path must have the same number of frames F."""
    from .pdb import pdb_to_atom14
    files = []
    for i in range(n_paths):
        stem = os.path.join(pdbdir, f"{name}_{i}")
        found = [stem + ext for ext in (".npy", ".pdb") if os.path.exists(stem + ext)]
        if not found:
            raise SystemExit(f"error: no path {i} of {name}: neither {stem}.npy nor .pdb exists")
        files.append(found[0])
    kept, F = [], None
    for i, path in enumerate(files):
        traj = np.load(path, mmap_mode="r") if path.endswith(".npy") else pdb_to_atom14(path, aatype)
        if F is None:
            F = int(traj.shape[0])
        if int(traj.shape[0]) != F or F < 1:
            raise SystemExit(f"error: ragged paths of {name}: {name}_{i} has {int(traj.shape[0])} frames, {name}_0 has {F}")
        kept.append(np.asarray(traj[strided_frames(F, stride)], np.float32))
    return np.stack(kept), F


def discretise(atom14, aatype, pkl, device):
    """The metastable-state dtraj (int32 device tensor [F]) of atom14 [F, L, 14, 3] by the pickle's tICA model, k-means centres
    and PCCA+ assignments: featurize -> project at the model's dim -> `kmeans_assign` -> lump (the reference's `discretize`)."""
    from . import analysis as A
    angles = A.featurize(A._device_f32(atom14, device), aatype)
    y = A.tica_transform(pkl["tica"], angles, pkl["tica"]["dim"])
    return A.lumped(y, pkl["kmeans"]["centers"], pkl["pcca"]["metastable_assignments"])[1]


def active_index_map(cmsm, nstates):
    """phi int32 [nstates]: a state's index in cmsm["active_set"]; a state outside it maps to argmax(pi) (module docstring)."""
    phi = np.full(int(nstates), int(np.argmax(cmsm["pi"])), np.int32)
    phi[np.asarray(cmsm["active_set"], np.int64)] = np.arange(len(cmsm["active_set"]), dtype=np.int32)
    return phi


def path_metrics(prob, ref_stateprobs, stateprobs):
    """(prob, valid_prob, valid_rate, JSD) of the reference's four lines (analyze_peptide_tps.py:80-83) from the paths'
    likelihood products; valid_prob is NaN when no product is positive."""
    from .analysis import jsd
    prob = np.asarray(prob, np.float64)
    pos = prob > 0
    return (float(prob.mean()), float(prob[pos].mean()) if pos.any() else float("nan"), float(pos.mean()),
            jsd(ref_stateprobs, stateprobs))


def _scatter(active_set, values, nstates):
    out = np.zeros(int(nstates))
    out[np.asarray(active_set, np.int64)] = values
    return out


def analyze_tps(name, pkl, records, gen_atom14, aatype, rep_atom14=None, n_samples=1000, seed=137, rep_lens=REP_LENS,
                rep_names=REP_NAMES, device="cuda"):
    """One peptide's result (module docstring) from the metadata, the kept frames of its paths [P, N, L, 14, 3] and, when there
    is one, the replica trajectory."""
    from . import analysis as A
    from . import msm as M
    cmsm = pkl["cmsm"]
    T, active = np.asarray(cmsm["transition_matrix"], np.float64), np.asarray(cmsm["active_set"], np.int64)
    nstates = int(np.asarray(pkl["pcca"]["memberships"]).shape[1])
    start_state, end_state = int(records[0]["start_state"]), int(records[0]["end_state"])
    if start_state not in active or end_state not in active:
        raise SystemExit(f"error: {name}: start state {start_state} / end state {end_state} outside the coarse MSM's active set")
    phi = active_index_map(cmsm, nstates)
    P, N = int(gen_atom14.shape[0]), int(gen_atom14.shape[1])
    out = dict(pkl)
    # the reference paths of the MD MSM
    ref_tp = A.tp_sample(T, phi[start_state], phi[end_state], N, n_samples, seed, 0, device=device)
    ref_stateprobs = M.state_probs(active[ref_tp], nstates)
    exact = M.bridge_exact(T, phi[start_state], phi[end_state], N)
    ref_exact = _scatter(active, exact["occupancy"], nstates)
    # the generated paths
    gen_tp = discretise(gen_atom14.reshape(P * N, *gen_atom14.shape[2:]), aatype, pkl, device).cpu().numpy().reshape(P, N)
    gen_stateprobs = M.state_probs(gen_tp, nstates)
    gen_prob = M.tp_likelihood(phi[gen_tp], T).prod(-1)
    out["gen_prob"], out["gen_valid_prob"], out["gen_valid_rate"], out["gen_JSD"] = path_metrics(gen_prob, ref_stateprobs, gen_stateprobs)
    # the replica baselines
    if rep_atom14 is not None:
        l_rep = discretise(rep_atom14, aatype, pkl, device)
        for i, (length, rep) in enumerate(zip(rep_lens, rep_names)):
            sampled = exact_rep = None
            C, _ = A.count_matrix(l_rep[:int(length)].contiguous(), cmsm["lag"], nstates)
            if C.sum() > 0:
                rep_msm = M.estimate_msm(C, cmsm["lag"])
                rep_active = np.asarray(rep_msm["active_set"], np.int64)
                if start_state in rep_active and end_state in rep_active:
                    rs, re = int(np.flatnonzero(rep_active == start_state)[0]), int(np.flatnonzero(rep_active == end_state)[0])
                    phi_rep = phi[rep_active]
                    try:
                        rep_tp, rep_prob = A.tp_sample(rep_msm["transition_matrix"], rs, re, N, n_samples, seed, 1 + i,
                                                       score=(T, phi_rep), device=device)
                    except ValueError as e:
                        print(f"{name}: {rep}: {e}", file=sys.stderr)
                    else:
                        sampled = path_metrics(rep_prob, ref_stateprobs, M.state_probs(rep_active[rep_tp], nstates))
                        ex = M.bridge_exact(rep_msm["transition_matrix"], rs, re, N, T, phi_rep)
                        exact_rep = (ex["prob"], ex["valid_prob"], ex["valid_rate"],
                                     A.jsd(ref_exact, _scatter(rep_active, ex["occupancy"], nstates)))
            if sampled is None:      # the reference's refusal values (analyze_peptide_tps.py:98-108)
                sampled, cheat, exact_rep = (0, 0, 0, 1), (np.nan,) * 4, (0, 0, 0, 1)
            else:
                cheat = sampled
            for key, a, b in zip(METRICS, sampled, cheat):
                out[f"{rep}_rep_{key}"], out[f"{rep}_repcheat_{key}"] = a, b
            for key, c in zip(METRICS, exact_rep):
                out[f"{rep}_rep_{key}_exact"] = c
    out["ref_stateprobs"], out["gen_stateprobs"], out["traj_len"] = ref_stateprobs, gen_stateprobs, N
    out["ref_stateprobs_exact"], out["gen_JSD_exact"] = ref_exact, A.jsd(ref_exact, gen_stateprobs)
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    if len(args.rep_lens) != len(args.rep_names):
        raise SystemExit(f"error: unequal --rep_lens ({len(args.rep_lens)}) and --rep_names ({len(args.rep_names)})")
    if args.stride < 1 or args.n_samples < 1:
        raise SystemExit("error: --stride and --n_samples must be >= 1")
    seqres = read_split(args.split)
    if args.pdb_id:
        names = list(args.pdb_id)
        unknown = [n for n in names if n not in seqres]
        if unknown:
            raise SystemExit(f"error: {unknown} not in {args.split}")
    else:
        names = [n for n in seqres if os.path.exists(os.path.join(args.pdbdir, f"{n}_metadata.json"))]
    from .geometry import restype_order
    loaded = {}
    for n in names:      # (every missing or ragged file is found before the first peptide is analysed, and before a device is needed)
        aat = np.array([restype_order[c] for c in seqres[n]])
        pkl, records = load_metadata(args.pdbdir, n)
        loaded[n] = (aat, pkl, records) + load_paths(args.pdbdir, n, len(records), aat, args.stride)
    print("number of peptides", len(names))
    import torch
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    os.makedirs(args.outdir, exist_ok=True)
    out = {}
    for n in names:
        aat, pkl, records, kept, F = loaded[n]
        rep_path = f"{args.repdir}/{n}{args.suffix}.npy"
        rep = np.load(rep_path, mmap_mode="r") if os.path.exists(rep_path) else None
        if rep is None:
            print(f"{n}: no replica baselines: {rep_path} does not exist", file=sys.stderr)
        out[n] = analyze_tps(n, pkl, records, kept, aat, rep, args.n_samples, args.seed, args.rep_lens, args.rep_names, device)
        with open(os.path.join(args.outdir, f"{n}.pkl"), "wb") as f:
            f.write(pickle.dumps(out[n]))
        print(f"{n}: {len(records)} paths of {F} frames, {out[n]['traj_len']} kept; gen_valid_rate {out[n]['gen_valid_rate']:.3f}, "
              f"gen_JSD {out[n]['gen_JSD']:.4f}")
    if args.save:
        with open(os.path.join(args.outdir, args.save_name), "wb") as f:
            f.write(pickle.dumps(out))
    return out


if __name__ == "__main__":
    main()
