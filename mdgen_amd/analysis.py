"""Analysis of sampled trajectories on the device: the parts of the reference's `scripts/analyze_peptide_sim.py` (:44-96) that
need no third-party estimator -- torsion angles of every frame, their 100-bin and 50 x 50 histograms with the Jensen-Shannon
distance against the MD trajectory, and the sin/cos autocovariance behind the "decorrelation" curves.  The kernels are
csrc/k_analysis.hip (`mdgen_traj_dihedrals`, `mdgen_traj_histograms`, `mdgen_traj_acov`, include/mdgen_amd.h); the arrays are on
the device when the sampler returns and stay there until the counts and curves, a few kilobytes, are copied back.

Out of scope: the tICA, k-means and MSM entries of the reference's result (`TICA-*`, `tica`, `msm`, `pcca`, ...), which pyemma's
estimators define; plots; reading or writing XTC files.

`torsion_features` imports without torch; the functions on tensors import torch and the library when they are called."""
from __future__ import annotations

import numpy as np

from .pdb import _checked_aatype, residue_tables

BINS_1D = 100                  # analyze_peptide_sim.py:52
BINS_2D = 50                   # :57
DEFAULT_PAIRS = ((1, 2), (3, 4))   # :56 `for i in [1, 3]: [:, i:i+2]`
MD_NLAG = 100000               # :68
NLAG = 1000                    # :87


# ---- features -------------------------------------------------------------------------------------------------------
def torsion_features(aatype, sidechains=True):
    """(labels, quad): the torsion angles of a sequence, `quad` int32 [NF, 4] holding each angle's four atoms as indices into
    one frame's L * 14 atom14 slots.

    Order: phi of residues 1 .. L-1 (C(i-1), N, CA, C), psi of residues 0 .. L-2 (N, CA, C, N(i+1)), then -- with `sidechains`
    -- chi1 of every residue that has one, then chi2, chi3, chi4 (`chi_atom_indices` / `chi_angles_mask` of
    data/residue_tables.npz).  Labels: "PHI 0 ALA 2", "PSI 0 ALA 1", "CHI1 0 LYS 2" -- chain 0, the residue's three-letter name,
    its number as this project's PDB writer numbers residues (from 0).

    This is the order and label form of pyemma's `add_backbone_torsions` + `add_sidechain_torsions` (mdgen/analysis.py
    get_featurizer) as the maintainers recall them; pyemma is not installed where this was written, so neither could be checked.
    The reference's scripts test labels only for the substrings PHI, PSI and CHI, which these keep.  mdtraj's chi5 of ARG is not in
    the residue tables and is left out."""
    t = residue_tables()
    aatype = _checked_aatype(aatype)
    res3 = [str(r) for r in t["restype_3"]]
    L = aatype.shape[0]
    labels, quad = [], []
    for i in range(1, L):
        labels.append(f"PHI 0 {res3[aatype[i]]} {i}")
        quad.append([(i - 1) * 14 + 2, i * 14, i * 14 + 1, i * 14 + 2])
    for i in range(L - 1):
        labels.append(f"PSI 0 {res3[aatype[i]]} {i}")
        quad.append([i * 14, i * 14 + 1, i * 14 + 2, (i + 1) * 14])
    if sidechains:
        for c in range(4):
            for i in range(L):
                aa = aatype[i]
                if t["chi_angles_mask"][aa][c] > 0:
                    labels.append(f"CHI{c + 1} 0 {res3[aa]} {i}")
                    quad.append([i * 14 + int(t["atom37_to_atom14"][aa][k]) for k in t["chi_atom_indices"][aa][c]])
    return labels, np.asarray(quad, np.int32).reshape(len(labels), 4)


def hist_edges(bins):
    """The fp64 bin edges of `np.histogram(range=(-np.pi, np.pi), bins=bins)`."""
    return np.linspace(-np.pi, np.pi, int(bins) + 1)


def jsd(p, q):
    """`scipy.spatial.distance.jensenshannon(p, q)` (natural logarithm) of two count vectors, restated in NumPy fp64: normalise,
    m = (p + q) / 2, sqrt((KL(p, m) + KL(q, m)) / 2).  A vector that sums to zero gives NaN, as scipy's does; a sum that rounding
    leaves just below zero counts as zero."""
    p = np.asarray(p, np.float64).ravel()
    q = np.asarray(q, np.float64).ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        p = p / p.sum()
        q = q / q.sum()
        m = (p + q) / 2.0

        def rel_entr(x, y):
            pos = x > 0
            return np.where(pos, x * np.log(np.where(pos, x, 1.0) / np.where(pos, y, 1.0)), np.where(x == 0, 0.0, np.inf))
        js = rel_entr(p, m).sum() + rel_entr(q, m).sum()
    return float(np.sqrt(max(js, 0.0) / 2.0)) if js == js else float("nan")


# ---- on device tensors ----------------------------------------------------------------------------------------------
def _device_f32(x, device=None):
    import torch
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.array(x, np.float32))   # (a copy: memory maps are read-only)
    if device is None and not x.is_cuda:
        from ._lib import MdgenError
        raise MdgenError("mdgen_amd.analysis runs on the GPU only (no CPU fallback): got a CPU tensor")
    return x.to(device=device if device is not None else x.device, dtype=torch.float32).contiguous()


def dihedrals_into(atom14, quad, angles) -> None:
    """One `mdgen_traj_dihedrals` call on atom14's device and current stream: atom14 (F, L, 14, 3) fp32 contiguous, `quad` a host
    int32 [NF, 4] array, `angles` (F, NF) fp32 written."""
    import torch
    from ._lib import launch, lib, ptr
    quad = np.ascontiguousarray(quad, np.int32).reshape(-1, 4)
    F, L, NF = int(atom14.shape[0]), int(atom14.shape[1]), int(quad.shape[0])
    if angles.numel() < F * NF:
        raise ValueError("angles needs F * NF elements")
    launch(lib.mdgen_traj_dihedrals, atom14, F, L, NF, ptr(atom14, torch.float32), quad.ctypes.data, ptr(angles, torch.float32))


def featurize(atom14, aatype, sidechains=True):
    """Torsion angles (F, NF) fp32 on the device of atom14 (F, L, 14, 3), a CUDA tensor, in `torsion_features`' order."""
    import torch
    aat = aatype.cpu().numpy() if hasattr(aatype, "cpu") else aatype
    _, quad = torsion_features(aat, sidechains)
    atom14 = _device_f32(atom14)
    if atom14.ndim != 4 or tuple(atom14.shape[-2:]) != (14, 3) or atom14.shape[1] != len(aat):
        raise ValueError(f"atom14 {tuple(atom14.shape)} / aatype {np.shape(aat)}: expected [F,L,14,3] and [L]")
    angles = torch.empty(atom14.shape[0], quad.shape[0], dtype=torch.float32, device=atom14.device)
    dihedrals_into(atom14, quad, angles)
    return angles


def histograms_into(angles, pairs, bins1, edges1, bins2, edges2, hist1, hist2, dropped) -> None:
    """One `mdgen_traj_histograms` call: angles (F, NF) fp32, `pairs` a host int32 [P, 2] array, edges fp64 device tensors;
    hist1 [NF, bins1], hist2 [P, bins2, bins2], dropped [NF + P] int64 are zeroed and filled."""
    import torch
    from ._lib import launch, lib, ptr
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    F, NF, P = int(angles.shape[0]), int(angles.shape[1]), int(pairs.shape[0])
    if hist1.numel() < NF * bins1 or hist2.numel() < P * bins2 * bins2 or dropped.numel() < NF + P:
        raise ValueError("hist1 needs NF * bins1 elements, hist2 P * bins2^2, dropped NF + P")
    if edges1.numel() != bins1 + 1 or edges2.numel() != bins2 + 1:
        raise ValueError("edges need bins + 1 elements")
    launch(lib.mdgen_traj_histograms, angles, F, NF, ptr(angles, torch.float32), int(bins1), ptr(edges1, torch.float64), P,
           pairs.ctypes.data, int(bins2), ptr(edges2, torch.float64), ptr(hist1, torch.int64), ptr(hist2, torch.int64),
           ptr(dropped, torch.int64))


def histograms(angles, pairs=(), bins1=BINS_1D, bins2=BINS_2D):
    """(hist1 [NF, bins1], hist2 [P, bins2, bins2], dropped [NF + P]) as int64 NumPy arrays: `np.histogram(x, bins=bins1,
    range=(-np.pi, np.pi))` of every column and `np.histogram2d` of every pair of columns, for fp64 x.  A value outside
    [-np.pi, np.pi] -- float32(pi) is one -- is in no bin, as for NumPy, and counted in `dropped` (features first, then pairs;
    a 2-D sample is dropped when either coordinate is)."""
    import torch
    angles = _device_f32(angles)
    dev = angles.device
    NF = int(angles.shape[1])
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    e1, e2 = torch.from_numpy(hist_edges(bins1)).to(dev), torch.from_numpy(hist_edges(bins2)).to(dev)
    h1 = torch.empty(NF, bins1, dtype=torch.int64, device=dev)
    h2 = torch.empty(P, bins2, bins2, dtype=torch.int64, device=dev)
    dr = torch.empty(NF + P, dtype=torch.int64, device=dev)
    histograms_into(angles, pairs, bins1, e1, bins2, e2, h1, h2, dr)
    return h1.cpu().numpy(), h2.cpu().numpy(), dr.cpu().numpy()


def acov_workspace_bytes(n, NF, nlag) -> int:
    import ctypes as C
    from ._lib import check, lib
    b = C.c_size_t()
    check(lib.mdgen_traj_acov_workspace_bytes(int(n), int(NF), int(nlag), C.byref(b)))
    return int(b.value)


def acov_into(angles, nlag, acov, mean_sin, mean_cos, workspace) -> None:
    """One `mdgen_traj_acov` call: angles (n, NF) fp32; acov [NF, nlag + 1], mean_sin [NF], mean_cos [NF] fp64 written;
    `workspace` a uint8 tensor of `acov_workspace_bytes(n, NF, nlag)`."""
    import torch
    from ._lib import launch, lib, ptr
    n, NF = int(angles.shape[0]), int(angles.shape[1])
    if acov.numel() < NF * (max(int(nlag), 0) + 1) or mean_sin.numel() < NF or mean_cos.numel() < NF:
        raise ValueError("acov needs NF * (nlag + 1) elements, the means NF")
    launch(lib.mdgen_traj_acov, angles, n, NF, int(nlag), ptr(angles, torch.float32), ptr(acov, torch.float64),
           ptr(mean_sin, torch.float64), ptr(mean_cos, torch.float64), ptr(workspace, torch.uint8), int(workspace.numel()))


def sincos_acov(angles, nlag):
    """(acov [NF, nlag + 1], mean_sin [NF], mean_cos [NF]) fp64 device tensors of angles (n, NF):
    acov[f, k] = (sum_t sin a_t sin a_{t+k} + cos a_t cos a_{t+k}) / (n - k), which is statsmodels' acovf(sin) + acovf(cos) with
    demean=False, adjusted=True.  nlag <= n - 1."""
    import torch
    angles = _device_f32(angles)
    n, NF = int(angles.shape[0]), int(angles.shape[1])
    dev = angles.device
    ws = torch.empty(max(acov_workspace_bytes(n, NF, nlag), 1), dtype=torch.uint8, device=dev)
    acov = torch.empty(NF, int(nlag) + 1, dtype=torch.float64, device=dev)
    ms, mc = torch.empty(NF, dtype=torch.float64, device=dev), torch.empty(NF, dtype=torch.float64, device=dev)
    acov_into(angles, nlag, acov, ms, mc, ws)
    return acov, ms, mc


def decorrelation(angles, nlag):
    """(acov - baseline) / (1 - baseline) as an fp64 device tensor [NF, nlag + 1], baseline = mean(sin)^2 + mean(cos)^2: the
    curve the reference stores (analyze_peptide_sim.py:68-96).  A constant series has baseline 1 and gives NaN (0 / 0), as the
    reference's expression does -- where the arithmetic is exact, as for the angle 0 of a degenerate quadruple; at another constant
    value both differences are rounding errors and so is their ratio, in the reference's expression alike."""
    acov, ms, mc = sincos_acov(angles, nlag)
    base = (ms * ms + mc * mc)[:, None]
    return (acov - base) / (1.0 - base)


def analyze(traj_atom14, ref_atom14, aatype, nlag=NLAG, ref_nlag=None, pairs=DEFAULT_PAIRS, decorr=True) -> dict:
    """The reference's per-peptide result for a sampled trajectory `traj_atom14` (F, L, 14, 3) against the MD trajectory
    `ref_atom14` (F_ref, L, 14, 3) -- a CUDA tensor, or an array that is copied to traj_atom14's device:

      "features"           the labels of `torsion_features(aatype)`
      "JSD"                {label: Jensen-Shannon distance of the two 100-bin histograms} and {"a|b": ... of the 50 x 50 ones} for
                           `pairs` of feature indices -- by default the reference's literal columns (1, 2) and (3, 4); pass
                           (phi_i, psi_i) index pairs for Ramachandran maps.  Pairs a short sequence does not have are dropped.
      "our_decorrelation"  {label: fp32 array [nlag + 1]} of `decorrelation` (nlag clamped to F - 1)
      "md_decorrelation"   the same of the MD trajectory, ref_nlag = min(100000, F_ref - 1) by default

    The last two only with `decorr`.  Plain Python and NumPy objects only.  The reference's tICA / MSM entries are not computed."""
    aat = _checked_aatype(aatype.cpu().numpy() if hasattr(aatype, "cpu") else aatype)
    traj = _device_f32(traj_atom14)
    ref = _device_f32(ref_atom14, traj.device)
    labels, _ = torsion_features(aat)
    NF = len(labels)
    out = {"features": list(labels), "JSD": {}}
    a_traj, a_ref = featurize(traj, aat), featurize(ref, aat)
    pairs = [(int(a), int(b)) for a, b in pairs if 0 <= int(a) < NF and 0 <= int(b) < NF]
    if NF:
        t1, t2, _ = histograms(a_traj, pairs)
        r1, r2, _ = histograms(a_ref, pairs)
        for i, lab in enumerate(labels):
            out["JSD"][lab] = jsd(r1[i], t1[i])
        for j, (a, b) in enumerate(pairs):
            out["JSD"]["|".join((labels[a], labels[b]))] = jsd(r2[j], t2[j])
    if decorr:
        n, n_ref = int(traj.shape[0]), int(ref.shape[0])
        k_ref = min(MD_NLAG if ref_nlag is None else int(ref_nlag), n_ref - 1)
        k = min(int(nlag), n - 1)
        md = decorrelation(a_ref, k_ref).cpu().numpy().astype(np.float32) if NF else np.zeros((0, k_ref + 1), np.float32)
        our = decorrelation(a_traj, k).cpu().numpy().astype(np.float32) if NF else np.zeros((0, k + 1), np.float32)
        out["our_decorrelation"] = {lab: our[i] for i, lab in enumerate(labels)}
        out["md_decorrelation"] = {lab: md[i] for i, lab in enumerate(labels)}
    return out
