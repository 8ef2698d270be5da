"""Analysis of sampled trajectories on the device: the parts of the reference's `scripts/analyze_peptide_sim.py` (:44-96) that
need no third-party estimator -- torsion angles of every frame, their 100-bin and 50 x 50 histograms with the Jensen-Shannon
distance against the MD trajectory, and the sin/cos autocovariance behind the "decorrelation" curves.  The kernels are
csrc/k_analysis.hip (`mdgen_traj_dihedrals`, `mdgen_traj_histograms`, `mdgen_traj_acov`, include/mdgen_amd.h); the arrays are on
the device when the sampler returns and stay there until the counts and curves, a few kilobytes, are copied back.

tICA (`tica_fit`, `tica_transform`; csrc/k_tica.hip: `mdgen_traj_lagged_moments`, `mdgen_traj_project`, `mdgen_traj_series_acov`,
`mdgen_traj_histograms_xy`) is a closed-form estimator and is built, opt-in (`analyze(tica=True)`): lagged second moments of the
cos/sin torsion features and the projection on the device, the D x D symmetric eigenproblem (D <= 128) in NumPy fp64 on the host.

k-means, the MSM and PCCA+ (`kmeans_fit`, `kmeans_assign`, `count_matrix`, `msm_entries`; csrc/k_msm.hip: `mdgen_traj_kmeans_assign`,
`mdgen_traj_kmeans_step`, `mdgen_traj_kmeans_pp`, `mdgen_traj_count_matrix`) are built, opt-in (`analyze(msm=True)`): k-means++ and
Lloyd's iteration on the MD trajectory's tICA projection and every count matrix on the device, the k x k estimators (k <= 256:
connected set, reversible maximum likelihood, PCCA+) in NumPy fp64 on the host, mdgen_amd/msm.py.  Every rule is restated there and
in the README; pyemma is not installed where this was written, and agreement with its seeded estimators is unverified.

Transition paths (`tp_sample`, `tp_sample_into`; csrc/k_tps.hip: `mdgen_tp_sample`): the reference's `sample_tp` -- paths of an MSM
pinned at a start and an end state -- and their likelihood under a second MSM, a thread per path; `md_msm`, the MD half of
`msm_entries`, is what `tps_inference --msm` builds its metadata from, and `python -m mdgen_amd.analyze_peptide_tps` scores the
sampled paths.

Out of scope: the Nelder-Mead refinement of PCCA+, pyemma object pickles (the estimators are stored as plain dicts), plots, TPT
fluxes; reading or writing XTC files.

`torsion_features` and `tica_solve` import without torch; the functions on tensors import torch and the library when they are
called."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .pdb import _checked_aatype, residue_tables

BINS_1D = 100                  # analyze_peptide_sim.py:52
BINS_2D = 50                   # :57
DEFAULT_PAIRS = ((1, 2), (3, 4))   # :56 `for i in [1, 3]: [:, i:i+2]`
MD_NLAG = 100000               # :68
NLAG = 1000                    # :87
TICA_LAG = 1000                # mdgen/analysis.py get_tica: pyemma.coordinates.tica(lag=1000, kinetic_map=True)
TICA_MAX_FEATURES = 64         # include/mdgen_amd.h mdgen_traj_lagged_moments: NF <= 64
KMEANS_K = 100                 # mdgen/analysis.py get_kmeans: cluster_kmeans(k=100, max_iter=100, fixed_seed=137)
KMEANS_MAX_ITER = 100
KMEANS_TOL = 1e-5              # pyemma's default tolerance
KMEANS_SEED = 137
KMEANS_MAX_DIM = 128           # include/mdgen_amd.h mdgen_traj_kmeans_*: d <= 128, k <= 256
KMEANS_MAX_K = 256
MSM_STATES = 10                # get_msm(nstates=10)
MD_MSM_LAG = 1000              # get_msm(lag=1000)
MSM_LAG = 10                   # analyze_peptide_sim.py --msm_lag


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


# ---- tICA -----------------------------------------------------------------------------------------------------------
# Features.  For angles (n, NF) in `torsion_features`' order, frame t has x_t in R^D, D = 2 NF, x[2j] = cos a_j, x[2j + 1] = sin a_j:
# pyemma's cossin=True interleaving as the maintainers recall it, unchecked like the label order; tICA's results do not depend on
# the order beyond rounding.  cos and sin are evaluated in fp64 and rounded to fp32 once.
# Moments at lag tau.  m = n - tau, X = x[0 .. m), Y = x[tau .. n): sx = sum X, sy = sum Y, cxx = X'X, cyy = Y'Y, cxy = X'Y, raw fp64.
class TicaModel(NamedTuple):
    """What `tica_solve` returns: `lag`; `mean` fp64 [D]; `eigenvalues` fp64 [rank], descending; `W` fp64 [D][rank], the kinetic
    map; `dim`, the number of components that hold `var_cutoff` of the kinetic variance; `rank` of C0."""
    lag: int
    mean: np.ndarray
    eigenvalues: np.ndarray
    W: np.ndarray
    dim: int
    rank: int

    def as_dict(self) -> dict:
        """Plain NumPy arrays and ints (what `analyze` stores: it unpickles without this package); `TicaModel(**d)` inverts it."""
        return {"lag": int(self.lag), "mean": np.array(self.mean), "eigenvalues": np.array(self.eigenvalues), "W": np.array(self.W),
                "dim": int(self.dim), "rank": int(self.rank)}


def tica_solve(m, sx, sy, cxx, cyy, cxy, epsilon=1e-6, var_cutoff=0.95, lag=0) -> TicaModel:
    """The estimator of `pyemma.coordinates.tica(lag, kinetic_map=True)` (defaults: reversible, var_cutoff 0.95, epsilon 1e-6) from
    the raw moments of m lagged pairs, in NumPy fp64:

      mu = (sx + sy) / 2m,  C0 = (cxx + cyy) / 2m - mu mu',  Ctau = (cxy + cxy') / 2m - mu mu'
      C0 = Q S Q'; the eigenvalues s > epsilon are kept, rank r is their number, L = Q_r S_r^(-1/2)
      L' Ctau L = R diag(lambda) R', lambda descending;  W = (L R) diag(lambda): the kinetic map
      sign: in every column of W the entry of largest magnitude is positive (the first such entry on ties)
      dim: the smallest d with sum_{i<d} lambda_i^2 / sum lambda_i^2 >= var_cutoff
      transform: (x_t - mu) W[:, :d]

    ValueError when rank < 2 (`TICA-0,1` needs two components)."""
    m = int(m)
    if m < 1:
        raise ValueError(f"tica_solve needs m >= 1 lagged pairs, got {m}")
    sx, sy = np.asarray(sx, np.float64).ravel(), np.asarray(sy, np.float64).ravel()
    D = sx.shape[0]
    cxx, cyy, cxy = (np.asarray(c, np.float64).reshape(D, D) for c in (cxx, cyy, cxy))
    mu = (sx + sy) / (2.0 * m)
    c0 = (cxx + cyy) / (2.0 * m) - np.outer(mu, mu)
    ct = (cxy + cxy.T) / (2.0 * m) - np.outer(mu, mu)
    s, q = np.linalg.eigh((c0 + c0.T) / 2.0)
    keep = np.flatnonzero(s > epsilon)[::-1]          # descending
    rank = int(keep.size)
    if rank < 2:
        raise ValueError(f"tICA needs a covariance of rank >= 2: rank {rank} of {D} features (eigenvalues above {epsilon:g})")
    L = q[:, keep] / np.sqrt(s[keep])
    mt = L.T @ ct @ L
    lam, r = np.linalg.eigh((mt + mt.T) / 2.0)
    lam, r = lam[::-1].copy(), r[:, ::-1]
    W = (L @ r) * lam
    big = np.argmax(np.abs(W), axis=0)                # (the first entry of largest magnitude)
    W = W * np.where(W[big, np.arange(rank)] < 0, -1.0, 1.0)
    share = np.cumsum(lam * lam) / np.sum(lam * lam)
    dim = int(min(np.searchsorted(share, var_cutoff, "left") + 1, rank))
    return TicaModel(int(lag), mu, lam, np.ascontiguousarray(W), dim, rank)


def _check_tica_shape(n, NF, lag):
    if not 1 <= NF <= TICA_MAX_FEATURES:
        raise ValueError(f"tICA takes 1 .. {TICA_MAX_FEATURES} torsions, got {NF}")
    if lag < 0 or lag > n - 1:
        raise ValueError(f"lag must be in 0 .. n - 1 (n = {n}, lag = {lag})")


def lagged_moments_workspace_bytes(n, NF, lag) -> int:
    import ctypes as C
    from ._lib import check, lib
    b = C.c_size_t()
    check(lib.mdgen_traj_lagged_moments_workspace_bytes(int(n), int(NF), int(lag), C.byref(b)))
    return int(b.value)


def lagged_moments_into(angles, lag, sx, sy, cxx, cyy, cxy, workspace) -> None:
    """One `mdgen_traj_lagged_moments` call: angles (n, NF) fp32; sx, sy [D], cxx, cyy, cxy [D, D] fp64 written, D = 2 NF;
    `workspace` a uint8 tensor of `lagged_moments_workspace_bytes(n, NF, lag)`."""
    import torch
    from ._lib import launch, lib, ptr
    n, NF = int(angles.shape[0]), int(angles.shape[1])
    D = 2 * NF
    _check_tica_shape(n, NF, int(lag))
    if sx.numel() < D or sy.numel() < D or min(cxx.numel(), cyy.numel(), cxy.numel()) < D * D:
        raise ValueError("sx, sy need D elements, cxx, cyy, cxy D * D")
    f64 = torch.float64
    launch(lib.mdgen_traj_lagged_moments, angles, n, NF, int(lag), ptr(angles, torch.float32), ptr(sx, f64), ptr(sy, f64),
           ptr(cxx, f64), ptr(cyy, f64), ptr(cxy, f64), ptr(workspace, torch.uint8), int(workspace.numel()))


def lagged_moments(angles, lag):
    """(sx [D], sy [D], cxx, cyy, cxy [D, D]) fp64 device tensors of angles (n, NF): the raw moments of the cos/sin features at
    `lag` (the section's head), 0 <= lag <= n - 1, 1 <= NF <= 64."""
    import torch
    angles = _device_f32(angles)
    n, NF = int(angles.shape[0]), int(angles.shape[1])
    _check_tica_shape(n, NF, int(lag))
    dev, D = angles.device, 2 * NF
    ws = torch.empty(max(lagged_moments_workspace_bytes(n, NF, lag), 1), dtype=torch.uint8, device=dev)
    sx, sy = torch.empty(D, dtype=torch.float64, device=dev), torch.empty(D, dtype=torch.float64, device=dev)
    cxx, cyy, cxy = (torch.empty(D, D, dtype=torch.float64, device=dev) for _ in range(3))
    lagged_moments_into(angles, lag, sx, sy, cxx, cyy, cxy, ws)
    return sx, sy, cxx, cyy, cxy


def tica_fit(angles, lag=TICA_LAG, epsilon=1e-6, var_cutoff=0.95) -> TicaModel:
    """tICA of angles (n, NF), a CUDA tensor: the moments on the device, `tica_solve` on the host.  ValueError, before any launch,
    when n - lag < 2 (one lagged pair has no covariance)."""
    n, NF, lag = int(angles.shape[0]), int(angles.shape[1]), int(lag)
    if lag < 0 or n - lag < 2:
        raise ValueError(f"tICA at lag {lag} needs at least lag + 2 frames, got {n}")
    _check_tica_shape(n, NF, lag)
    parts = [p.cpu().numpy() for p in lagged_moments(angles, lag)]
    return tica_solve(n - lag, *parts, epsilon=epsilon, var_cutoff=var_cutoff, lag=lag)


def project_into(angles, mean, W, out) -> None:
    """One `mdgen_traj_project` call: angles (n, NF) fp32, mean [D] and W [D, d] fp32 device tensors, out (n, d) fp32 written."""
    import torch
    from ._lib import launch, lib, ptr
    n, NF = int(angles.shape[0]), int(angles.shape[1])
    D = 2 * NF
    d = int(W.numel() // D) if D else 0
    if not 1 <= NF <= TICA_MAX_FEATURES:
        raise ValueError(f"tICA takes 1 .. {TICA_MAX_FEATURES} torsions, got {NF}")
    if W.ndim != 2 or W.shape[0] != D or not 1 <= d <= D:
        raise ValueError(f"W {tuple(W.shape)}: expected [D, d] with D = {D} and 1 <= d <= D")
    if mean.numel() != D or out.numel() < n * d:
        raise ValueError("mean needs D elements, out n * d")
    f32 = torch.float32
    launch(lib.mdgen_traj_project, angles, n, NF, d, ptr(angles, f32), ptr(mean, f32), ptr(W, f32), ptr(out, f32))


def tica_transform(model, angles, dim=None):
    """(n, d) fp32 device tensor: (x_t - mean) W[:, :d] of angles (n, NF), d = `dim` or the model's; `mean` and `W` are rounded to
    fp32 once, the subtraction comes first, then fp32 FMAs over the features in ascending order.  `model`: a TicaModel or its dict."""
    import torch
    if isinstance(model, dict):
        model = TicaModel(**model)
    d = int(model.dim if dim is None else dim)
    if not 1 <= d <= model.rank:
        raise ValueError(f"dim must be in 1 .. rank = {model.rank}, got {d}")
    if 2 * int(angles.shape[1]) != model.mean.shape[0]:
        raise ValueError(f"the model has {model.mean.shape[0]} features, the angles give {2 * int(angles.shape[1])}")
    angles = _device_f32(angles)
    dev = angles.device
    mean = torch.from_numpy(np.asarray(model.mean, np.float64).astype(np.float32)).to(dev)
    W = torch.from_numpy(np.ascontiguousarray(np.asarray(model.W, np.float64)[:, :d]).astype(np.float32)).to(dev)
    out = torch.empty(int(angles.shape[0]), d, dtype=torch.float32, device=dev)
    project_into(angles, mean, W, out)
    return out


def series_acov_workspace_bytes(n, NS, nlag) -> int:
    import ctypes as C
    from ._lib import check, lib
    b = C.c_size_t()
    check(lib.mdgen_traj_series_acov_workspace_bytes(int(n), int(NS), int(nlag), C.byref(b)))
    return int(b.value)


def series_acov_into(x, nlag, acov, mean, workspace) -> None:
    """One `mdgen_traj_series_acov` call: x (n, NS) fp32; acov [NS, nlag + 1], mean [NS] fp64 written; `workspace` a uint8 tensor
    of `series_acov_workspace_bytes(n, NS, nlag)`."""
    import torch
    from ._lib import launch, lib, ptr
    n, NS = int(x.shape[0]), int(x.shape[1])
    if acov.numel() < NS * (max(int(nlag), 0) + 1) or mean.numel() < NS:
        raise ValueError("acov needs NS * (nlag + 1) elements, mean NS")
    launch(lib.mdgen_traj_series_acov, x, n, NS, int(nlag), ptr(x, torch.float32), ptr(acov, torch.float64), ptr(mean, torch.float64),
           ptr(workspace, torch.uint8), int(workspace.numel()))


def series_acov(x, nlag):
    """(acov [NS, nlag + 1], mean [NS]) fp64 device tensors of the series x (n, NS) -- or (n,), one series:
    acov[s, k] = sum_{t < n - k} x_t x_{t+k} / (n - k), statsmodels' acovf(demean=False, adjusted=True).  nlag <= n - 1."""
    import torch
    x = _device_f32(x)
    if x.ndim == 1:
        x = x[:, None].contiguous()
    n, NS = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    ws = torch.empty(max(series_acov_workspace_bytes(n, NS, nlag), 1), dtype=torch.uint8, device=dev)
    acov = torch.empty(NS, int(nlag) + 1, dtype=torch.float64, device=dev)
    mean = torch.empty(NS, dtype=torch.float64, device=dev)
    series_acov_into(x, nlag, acov, mean, ws)
    return acov, mean


def range_edges(lo, hi, bins):
    """The fp64 bin edges of `np.histogram(range=(lo, hi), bins=bins)`; a degenerate range lo == hi becomes (lo - 0.5, hi + 0.5),
    as NumPy makes it."""
    lo, hi = float(lo), float(hi)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, int(bins) + 1)


def histograms_xy_into(values, pairs, bins, edges_x, edges_y, hist2, dropped) -> None:
    """One `mdgen_traj_histograms_xy` call: values (F, NC) fp32, `pairs` a host int32 [P, 2] array, edges_x and edges_y fp64
    [P, bins + 1] device tensors; hist2 [P, bins, bins] and dropped [P] int64 are zeroed and filled."""
    import torch
    from ._lib import launch, lib, ptr
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    F, NC, P = int(values.shape[0]), int(values.shape[1]), int(pairs.shape[0])
    if hist2.numel() < P * bins * bins or dropped.numel() < P:
        raise ValueError("hist2 needs P * bins^2 elements, dropped P")
    if edges_x.numel() != P * (bins + 1) or edges_y.numel() != P * (bins + 1):
        raise ValueError("edges need P * (bins + 1) elements")
    launch(lib.mdgen_traj_histograms_xy, values, F, NC, ptr(values, torch.float32), P, pairs.ctypes.data, int(bins),
           ptr(edges_x, torch.float64), ptr(edges_y, torch.float64), ptr(hist2, torch.int64), ptr(dropped, torch.int64))


def histogram2d_xy(values, pairs, bins, ranges):
    """(hist2 [P, bins, bins], dropped [P]) int64 NumPy arrays: `np.histogram2d(x, y, bins=bins, range=ranges[p])` of the columns
    (x, y) = pairs[p] of values (F, NC), widened to fp64, with `ranges[p]` = ((x_lo, x_hi), (y_lo, y_hi)) of its own per pair."""
    import torch
    values = _device_f32(values)
    dev = values.device
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    if len(ranges) != P:
        raise ValueError("one ((x_lo, x_hi), (y_lo, y_hi)) per pair")
    ex = np.stack([range_edges(*r[0], bins) for r in ranges]) if P else np.zeros((0, bins + 1))
    ey = np.stack([range_edges(*r[1], bins) for r in ranges]) if P else np.zeros((0, bins + 1))
    h2 = torch.empty(P, bins, bins, dtype=torch.int64, device=dev)
    dr = torch.empty(P, dtype=torch.int64, device=dev)
    histograms_xy_into(values, pairs, int(bins), torch.from_numpy(ex).to(dev), torch.from_numpy(ey).to(dev), h2, dr)
    return h2.cpu().numpy(), dr.cpu().numpy()


def _hist1d_range(values, column, lo, hi, bins):
    """`np.histogram(values[:, column], bins=bins, range=(lo, hi))[0]` through `mdgen_traj_histograms`."""
    import torch
    col = values[:, column:column + 1].contiguous()
    dev = col.device
    e = torch.from_numpy(range_edges(lo, hi, bins)).to(dev)
    h1 = torch.empty(1, bins, dtype=torch.int64, device=dev)
    dr = torch.empty(1, dtype=torch.int64, device=dev)
    histograms_into(col, np.zeros((0, 2), np.int32), bins, e, 1, e[:2].contiguous(), h1, h1[:0], dr)
    return h1[0].cpu().numpy()


def tica_entries(a_traj, a_ref, lag=TICA_LAG, nlag=NLAG, ref_nlag=None, decorr=True, projections=False) -> dict:
    """The tICA part of the reference's result (analyze_peptide_sim.py:104-150) from the two angle tensors: fit on the MD angles,
    transform both.  {"TICA-0", "TICA-0,1"} JSDs, "model" (`TicaModel.as_dict()`) and, with `decorr`, "md_tica" / "our_tica": the
    autocovariance of component 0, fp32, neither demeaned nor normalised, as the reference stores it.  With `projections` also "y_ref" /
    "y_traj", the (n, max(dim, 2)) fp32 device tensors of `tica_transform`."""
    import torch
    model = tica_fit(a_ref, lag)
    d = max(model.dim, 2)
    y_ref, y_traj = tica_transform(model, a_ref, d), tica_transform(model, a_traj, d)
    lo = torch.minimum(y_ref[:, :2].amin(0), y_traj[:, :2].amin(0)).double().cpu().numpy()   # (fp32 widened: plumbing)
    hi = torch.maximum(y_ref[:, :2].amax(0), y_traj[:, :2].amax(0)).double().cpu().numpy()
    out = {"model": model.as_dict()}
    out["TICA-0"] = jsd(_hist1d_range(y_ref, 0, lo[0], hi[0], BINS_1D), _hist1d_range(y_traj, 0, lo[0], hi[0], BINS_1D))
    rng = [((lo[0], hi[0]), (lo[1], hi[1]))]
    r2, _ = histogram2d_xy(y_ref, [(0, 1)], BINS_2D, rng)
    t2, _ = histogram2d_xy(y_traj, [(0, 1)], BINS_2D, rng)
    out["TICA-0,1"] = jsd(r2[0], t2[0])
    if decorr:
        n, n_ref = int(y_traj.shape[0]), int(y_ref.shape[0])
        k_ref = min(MD_NLAG if ref_nlag is None else int(ref_nlag), n_ref - 1)
        k = min(int(nlag), n - 1)
        out["md_tica"] = series_acov(y_ref[:, 0].contiguous(), k_ref)[0][0].cpu().numpy().astype(np.float32)
        out["our_tica"] = series_acov(y_traj[:, 0].contiguous(), k)[0][0].cpu().numpy().astype(np.float32)
    if projections:
        out["y_ref"], out["y_traj"] = y_ref, y_traj
    return out


# ---- k-means, count matrices, the MSM chain --------------------------------------------------------------------------
# Distance: dist2(x, c) = sum_j (x_j - c_j)^2, the fp32 difference and fp32 FMAs over j ascending; the nearest centre is the one of
# smallest dist2, ties to the lowest index.  x (n, d) fp32 with 1 <= d <= 128, centres fp32 [k, d] with 1 <= k <= 256.
def _check_kmeans_shape(n, d, k):
    if n < 1:
        raise ValueError("k-means needs at least one point")
    if not 1 <= d <= KMEANS_MAX_DIM:
        raise ValueError(f"k-means takes 1 .. {KMEANS_MAX_DIM} dimensions, got {d}")
    if not 1 <= k <= KMEANS_MAX_K:
        raise ValueError(f"k-means takes 1 .. {KMEANS_MAX_K} centres, got {k}")


def _workspace_bytes(fn, *shape) -> int:
    import ctypes as C
    from ._lib import check
    b = C.c_size_t()
    check(fn(*[int(v) for v in shape], C.byref(b)))
    return int(b.value)


def kmeans_step_workspace_bytes(n, d, k) -> int:
    from ._lib import lib
    return _workspace_bytes(lib.mdgen_traj_kmeans_step_workspace_bytes, n, d, k)


def kmeans_pp_workspace_bytes(n, d, k) -> int:
    from ._lib import lib
    return _workspace_bytes(lib.mdgen_traj_kmeans_pp_workspace_bytes, n, d, k)


def kmeans_assign_into(x, centers, assign, dist2=None) -> None:
    """One `mdgen_traj_kmeans_assign` call: x (n, d) and centers (k, d) fp32; assign int32 [n] and, when given, dist2 fp32 [n]
    written."""
    import torch
    from ._lib import launch, lib, ptr
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(centers.shape[0])
    _check_kmeans_shape(n, d, k)
    if centers.ndim != 2 or int(centers.shape[1]) != d or assign.numel() < n or (dist2 is not None and dist2.numel() < n):
        raise ValueError("centers must be [k, d]; assign and dist2 need n elements")
    launch(lib.mdgen_traj_kmeans_assign, x, n, d, k, ptr(x, torch.float32), ptr(centers, torch.float32), ptr(assign, torch.int32),
           ptr(dist2, torch.float32))


def kmeans_assign(x, centers, dist2=False):
    """The index of every point's nearest centre, an int32 device tensor [n] -- the discretisation of a trajectory, what
    `kmeans.transform` gives the reference; with `dist2` also the fp32 squared distances."""
    import torch
    x = _device_f32(x)
    centers = _device_f32(centers, x.device)
    assign = torch.empty(int(x.shape[0]), dtype=torch.int32, device=x.device)
    d2 = torch.empty(int(x.shape[0]), dtype=torch.float32, device=x.device) if dist2 else None
    kmeans_assign_into(x, centers, assign, d2)
    return (assign, d2) if dist2 else assign


def kmeans_step_into(x, centers, assign, sums, counts, cost, state, tol, workspace) -> None:
    """One `mdgen_traj_kmeans_step` call, a Lloyd iteration (include/mdgen_amd.h): centers (k, d) fp32 updated in place; assign
    int32 [n], sums fp64 [k, d], counts int64 [k] written; cost fp64 [2] and state int32 [2] (done flag, steps taken) carried from
    step to step on the device -- zero both before the first.  A step that finds the flag set changes nothing."""
    import torch
    from ._lib import launch, lib, ptr
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(centers.shape[0])
    _check_kmeans_shape(n, d, k)
    if centers.ndim != 2 or int(centers.shape[1]) != d or assign.numel() < n or sums.numel() < k * d or counts.numel() < k:
        raise ValueError("centers must be [k, d]; assign needs n elements, sums k * d, counts k")
    if cost.numel() < 2 or state.numel() < 2:
        raise ValueError("cost and state need 2 elements")
    launch(lib.mdgen_traj_kmeans_step, x, n, d, k, ptr(x, torch.float32), ptr(centers, torch.float32), ptr(assign, torch.int32),
           ptr(sums, torch.float64), ptr(counts, torch.int64), ptr(cost, torch.float64), ptr(state, torch.int32), float(tol),
           ptr(workspace, torch.uint8), int(workspace.numel()))


def kmeans_pp_into(x, k, u, r0, r1, chosen, mind2, workspace) -> None:
    """One `mdgen_traj_kmeans_pp` call: rounds r0 .. r1 - 1 of k-means++ on x (n, d) with the host uniforms u fp64 [k];
    chosen int64 [k] and mind2 fp32 [n] live on the device between rounds."""
    import torch
    from ._lib import launch, lib, ptr
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(k)
    _check_kmeans_shape(n, d, k)
    u = np.ascontiguousarray(u, np.float64).ravel()
    if u.shape[0] < k or chosen.numel() < k or mind2.numel() < n:
        raise ValueError("u and chosen need k elements, mind2 n")
    launch(lib.mdgen_traj_kmeans_pp, x, n, d, k, ptr(x, torch.float32), u.ctypes.data, int(r0), int(r1), ptr(chosen, torch.int64),
           ptr(mind2, torch.float32), ptr(workspace, torch.uint8), int(workspace.numel()))


def kmeans_pp(x, k, u):
    """k-means++ seeding in one call: the int64 device tensor [k] of chosen point indices.  Round 0 takes floor(u[0] n); round r
    takes the smallest i with sum_{t <= i} mind2[t] > u[r] sum_t mind2[t], mind2 the squared distance to the nearest point chosen
    so far (floor(u[r] n) when that sum is zero)."""
    import torch
    x = _device_f32(x)
    n, d = int(x.shape[0]), int(x.shape[1])
    _check_kmeans_shape(n, d, int(k))
    chosen = torch.zeros(int(k), dtype=torch.int64, device=x.device)
    mind2 = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(kmeans_pp_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device=x.device)
    kmeans_pp_into(x, k, u, 0, int(k), chosen, mind2, ws)
    return chosen


def kmeans_fit(x, k=KMEANS_K, max_iter=KMEANS_MAX_ITER, tol=KMEANS_TOL, seed=KMEANS_SEED) -> dict:
    """k-means of x (n, d), a CUDA tensor, as the reference asks for it (`cluster_kmeans(k=100, max_iter=100, fixed_seed=137)`),
    restated: u = np.random.default_rng(seed).random(k) drives k-means++ (`kmeans_pp`), the rows x[chosen] are the initial
    centres, then at most `max_iter` Lloyd steps (`kmeans_step_into`), stopping after the step whose cost differs from the previous
    step's by at most tol * cost.  All steps are launched back to back -- the done flag lives on the device -- and read back once.

    {"centers" fp32 [k, d], "dim" d, "steps", "cost" (of the last step, measured before its update), "cost_history" fp64 [steps],
    "seed", "chosen" int64 [k]}.  ValueError when k > n."""
    import torch
    x = _device_f32(x)
    n, d, k = int(x.shape[0]), int(x.shape[1]), int(k)
    _check_kmeans_shape(n, d, k)
    if k > n:
        raise ValueError(f"k-means with {k} centres needs at least as many points, got {n}")
    dev = x.device
    u = np.random.default_rng(int(seed)).random(k)
    chosen = kmeans_pp(x, k, u)
    centers = x.index_select(0, chosen).contiguous()
    assign = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.empty(k, d, dtype=torch.float64, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    cost = torch.zeros(2, dtype=torch.float64, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    history = torch.zeros(max(int(max_iter), 1), dtype=torch.float64, device=dev)
    ws = torch.empty(max(kmeans_step_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device=dev)
    for i in range(int(max_iter)):
        kmeans_step_into(x, centers, assign, sums, counts, cost, state, tol, ws)
        history[i:i + 1].copy_(cost[:1])
    steps = int(state.cpu()[1])
    history = history.cpu().numpy()[:steps].copy()
    return {"centers": centers.cpu().numpy(), "dim": d, "steps": steps, "cost": float(history[-1]) if steps else 0.0,
            "cost_history": history, "seed": int(seed), "chosen": chosen.cpu().numpy()}


def count_matrix_into(dtraj, lag, k, counts, dropped) -> None:
    """One `mdgen_traj_count_matrix` call: dtraj int32 [n]; counts int64 [k, k] and dropped int64 [1] are zeroed and filled."""
    import torch
    from ._lib import launch, lib, ptr
    if not 1 <= int(k) <= KMEANS_MAX_K:
        raise ValueError(f"a count matrix takes 1 .. {KMEANS_MAX_K} states, got {k}")
    if int(lag) < 0:
        raise ValueError(f"lag must be >= 0, got {lag}")
    if counts.numel() < int(k) * int(k) or dropped.numel() < 1:
        raise ValueError("counts needs k * k elements, dropped 1")
    launch(lib.mdgen_traj_count_matrix, dtraj, int(dtraj.numel()), int(lag), int(k), ptr(dtraj, torch.int32), ptr(counts, torch.int64),
           ptr(dropped, torch.int64))


def count_matrix(dtraj, lag, k):
    """(counts int64 [k, k], dropped) as a NumPy array and an int: counts[i, j] = #{t < n - lag: dtraj[t] = i, dtraj[t + lag] = j},
    the sliding-window count of pyemma's default; a pair with a state outside 0 .. k - 1 is counted in `dropped`.  dtraj: an int32
    CUDA tensor [n]."""
    import torch
    dev = dtraj.device
    counts = torch.empty(int(k), int(k), dtype=torch.int64, device=dev)
    dropped = torch.empty(1, dtype=torch.int64, device=dev)
    count_matrix_into(dtraj.contiguous(), lag, k, counts, dropped)
    return counts.cpu().numpy(), int(dropped.cpu()[0])


def _filled(active_set, values, nstates, base):
    """The reference's `np.eye(nstates)` / `np.zeros(nstates)` filled through an estimator's active set
    (analyze_peptide_sim.py:169-179)."""
    out = np.array(base, np.float64)
    active_set = np.asarray(active_set)
    if out.ndim == 2:
        out[np.ix_(active_set, active_set)] = values
    else:
        out[active_set] = values
    return out


def md_msm(y_ref, k=KMEANS_K, nstates=MSM_STATES, md_lag=MD_MSM_LAG, seed=KMEANS_SEED):
    """The MD half of `msm_entries` -- its steps 1 and 3 .. 6, which need no sampled trajectory -- from the MD trajectory's tICA
    projection y_ref (n, d), an fp32 CUDA tensor: (entries, d_ref).  `entries`: {"kmeans", "msm", "pcca", "cmsm"}, plain dicts;
    `d_ref`: the MD trajectory's microstate dtraj, an int32 device tensor [n].  The ValueErrors are `msm_entries`'."""
    import torch
    from . import msm as M
    k, nstates = int(k), int(nstates)
    if not 1 <= nstates <= k:
        raise ValueError(f"{nstates} metastable states of {k} microstates")
    y_ref = _device_f32(y_ref)
    km = kmeans_fit(y_ref, k, seed=seed)
    centers = torch.from_numpy(km["centers"]).to(y_ref.device)
    d_ref = kmeans_assign(y_ref, centers)
    C, _ = count_matrix(d_ref, md_lag, k)
    if C.sum() == 0:
        raise ValueError(f"no transition counts: the MD trajectory has {int(y_ref.shape[0])} frames, the MSM lag is {int(md_lag)}")
    model = M.estimate_msm(C, md_lag)
    if len(model["active_set"]) != k:
        raise ValueError(f"only {len(model['active_set'])} of {k} microstates are in the MSM's connected set at lag {int(md_lag)}")
    pc = M.pcca(model["transition_matrix"], model["pi"], nstates)
    lump = np.zeros((k, nstates), np.int64)
    lump[np.arange(k), pc["metastable_assignments"]] = 1
    cmsm = M.estimate_msm(lump.T @ C @ lump, md_lag)
    return {"kmeans": {key: km[key] for key in ("centers", "dim", "steps", "cost", "seed")}, "msm": model, "pcca": pc, "cmsm": cmsm}, d_ref


def lumped(y, centers, meta):
    """The metastable-state dtraj of the projection y (n, d): `kmeans_assign` by the fitted `centers`, then the PCCA+ assignment
    `meta` [k] of every microstate -- the reference's `discretize`.  (microstates, metastable states), int32 device tensors [n]."""
    import torch
    y = _device_f32(y)
    d = kmeans_assign(y, torch.from_numpy(np.asarray(centers, np.float32)).to(y.device))
    meta_dev = torch.from_numpy(np.asarray(meta).astype(np.int32)).to(y.device)
    return d, meta_dev[d.long()].contiguous()


def msm_entries(y_traj, y_ref, k=KMEANS_K, nstates=MSM_STATES, md_lag=MD_MSM_LAG, traj_lag=MSM_LAG, traj_msm=True, seed=KMEANS_SEED,
                name=None) -> dict:
    """The k-means / MSM / PCCA+ part of the reference's result (analyze_peptide_sim.py:153-197; mdgen/analysis.py get_kmeans,
    get_msm, discretize) from the tICA projections y_ref (MD) and y_traj (sampled), (n, d) fp32 CUDA tensors:

      1. `kmeans_fit(y_ref, k, seed=seed)`;  2. both trajectories discretised (`kmeans_assign`);
      3. the MD dtraj's count matrix at `md_lag` (device);  4. `msm.estimate_msm` -- ValueError unless all k microstates are in
      its active set, as the reference asserts;  5. `msm.pcca(nstates)`;
      6. the coarse MSM from the lumped count matrix M' C M (M the k x nstates indicator of the assignments: exactly the count
         matrix of the lumped dtraj);  7. both dtrajs lumped, their occupancies from lag-0 counts (device);
      8. with `traj_msm`: the lumped sampled dtraj counted at `traj_lag` (device) and `msm.estimate_msm`.  When that alone fails
         (no transition counts), its three entries are left out and `name` is written to stderr.

    Steps 1 and 3 .. 6 are `md_msm`'s.  Keys, in order: kmeans, msm, pcca, cmsm, traj_metastable_probs, ref_metastable_probs,
    msm_transition_matrix, pcca_pi, msm_pi, and traj_msm, traj_transition_matrix, traj_pi.  Estimators are plain dicts of NumPy
    arrays and ints."""
    import sys
    import torch
    from . import msm as M
    k, nstates = int(k), int(nstates)
    if not 1 <= nstates <= k:
        raise ValueError(f"{nstates} metastable states of {k} microstates")
    y_ref = _device_f32(y_ref)
    y_traj = _device_f32(y_traj, y_ref.device)
    out, d_ref = md_msm(y_ref, k, nstates, md_lag, seed)
    pc, cmsm = out["pcca"], out["cmsm"]
    meta_dev = torch.from_numpy(pc["metastable_assignments"].astype(np.int32)).to(y_ref.device)
    l_ref = meta_dev[d_ref.long()].contiguous()
    _, l_traj = lumped(y_traj, out["kmeans"]["centers"], pc["metastable_assignments"])
    out["traj_metastable_probs"] = np.diag(count_matrix(l_traj, 0, nstates)[0]) / float(l_traj.numel())
    out["ref_metastable_probs"] = np.diag(count_matrix(l_ref, 0, nstates)[0]) / float(l_ref.numel())
    out["msm_transition_matrix"] = _filled(cmsm["active_set"], cmsm["transition_matrix"], nstates, np.eye(nstates))
    out["pcca_pi"] = pc["pi_coarse"]
    out["msm_pi"] = _filled(cmsm["active_set"], cmsm["pi"], nstates, np.zeros(nstates))
    if traj_msm:
        try:
            Ct, _ = count_matrix(l_traj, traj_lag, nstates)
            if Ct.sum() == 0:
                raise ValueError(f"no transition counts: {int(l_traj.numel())} sampled frames, lag {int(traj_lag)}")
            tm = M.estimate_msm(Ct, traj_lag)
        except ValueError as e:
            print(f"{name if name is not None else 'sampled trajectory'}: no traj_msm entries: {e}", file=sys.stderr)
        else:
            out["traj_msm"] = tm
            out["traj_transition_matrix"] = _filled(tm["active_set"], tm["transition_matrix"], nstates, np.eye(nstates))
            out["traj_pi"] = _filled(tm["active_set"], tm["pi"], nstates, np.zeros(nstates))
    return out


# ---- transition paths ------------------------------------------------------------------------------------------------
TP_MAX_STATES = 64             # include/mdgen_amd.h mdgen_tp_sample: k, kb <= 64, 2 <= N <= 4096
TP_MAX_LEN = 4096


def _check_tp_shape(n_samples, N, k, start, end):
    if n_samples < 1:
        raise ValueError(f"at least one path, got {n_samples}")
    if not 2 <= N <= TP_MAX_LEN:
        raise ValueError(f"a path has 2 .. {TP_MAX_LEN} frames, got {N}")
    if not 1 <= k <= TP_MAX_STATES:
        raise ValueError(f"the bridge sampler takes 1 .. {TP_MAX_STATES} states, got {k}")
    if not (0 <= start < k and 0 <= end < k):
        raise ValueError(f"start {start} / end {end} outside the {k} states")


def tp_sample_into(Ta, Ba, start, end, seed, stream, paths, sample_base=0, Tb=None, Bb=None, phi=None, prob=None) -> None:
    """One `mdgen_tp_sample` call on paths' device and current stream: Ta [k, k] and Ba [N, k] fp64 device tensors
    (`msm.bridge_table(Ta, end, N)`); paths int32 [n_samples, N] written.  With the scoring set -- Tb [kb, kb], Bb [N, kb]
    (`msm.bridge_table(Tb, phi[end], N)`) fp64 device tensors, `phi` a host int32 [k] array -- also prob fp64 [n_samples]."""
    import torch
    from ._lib import launch, lib, ptr
    n_samples, N, k = int(paths.shape[0]), int(paths.shape[1]), int(Ta.shape[0])
    _check_tp_shape(n_samples, N, k, int(start), int(end))
    f64 = torch.float64
    if Ta.ndim != 2 or int(Ta.shape[1]) != k or Ba.numel() != N * k:
        raise ValueError("Ta must be [k, k], Ba [N, k]")
    kb, phi_p = 0, None
    if Tb is not None:
        kb = int(Tb.shape[0])
        phi = np.ascontiguousarray(phi, np.int32).ravel()
        if not 1 <= kb <= TP_MAX_STATES or Tb.ndim != 2 or int(Tb.shape[1]) != kb or Bb.numel() != N * kb or phi.shape[0] != k:
            raise ValueError(f"Tb must be [kb, kb] with kb <= {TP_MAX_STATES}, Bb [N, kb], phi [k]")
        if prob is None or prob.numel() < n_samples:
            raise ValueError("prob needs n_samples elements")
        phi_p = phi.ctypes.data
    launch(lib.mdgen_tp_sample, paths, n_samples, N, k, ptr(Ta, f64), ptr(Ba, f64), int(start), int(end), int(seed) % (1 << 64),
           int(stream) % (1 << 32), int(sample_base) % (1 << 64), kb, ptr(Tb, f64) if kb else None, ptr(Bb, f64) if kb else None,
           phi_p, ptr(paths, torch.int32), ptr(prob, f64) if kb else None)


def tp_sample(Ta, start, end, N, n_samples, seed, stream, score=None, sample_base=0, device=None):
    """The reference's `sample_tp(Ta, start, end, N, n_samples)` on the device: paths int32 [n_samples, N] as a NumPy array, every
    path a draw of the chain Ta (fp64 [k, k], matrix indices) pinned at `start` and `end`; path s depends on (seed, stream,
    sample_base + s) alone (include/mdgen_amd.h mdgen_tp_sample states the draw).  With `score` = (Tb, phi) -- a scoring matrix and
    the index map from Ta's states into Tb's -- (paths, prob): prob fp64 [n_samples] = `msm.tp_likelihood(phi[paths], Tb).prod(-1)`.
    ValueError when `end` cannot be reached from `start` in N - 1 steps."""
    import torch
    from . import msm as M
    Ta = np.ascontiguousarray(Ta, np.float64)
    k, N, n_samples, start, end = Ta.shape[0], int(N), int(n_samples), int(start), int(end)
    if Ta.ndim != 2 or Ta.shape[1] != k:
        raise ValueError(f"transition matrix {Ta.shape}: expected [k, k]")
    _check_tp_shape(n_samples, N, k, start, end)
    Ba = M.bridge_table(Ta, end, N)
    if not Ba[N - 1, start] > 0:
        raise ValueError(f"end state not reachable in N - 1 steps: (Ta^{N - 1})[{start}, {end}] = {Ba[N - 1, start]}")
    if score is not None:
        Tb, phi = np.ascontiguousarray(score[0], np.float64), np.ascontiguousarray(score[1], np.int32).ravel()
        if Tb.ndim != 2 or Tb.shape[0] != Tb.shape[1] or not 1 <= Tb.shape[0] <= TP_MAX_STATES:
            raise ValueError(f"scoring matrix {Tb.shape}: expected [kb, kb], kb <= {TP_MAX_STATES}")
        if phi.shape[0] != k or phi.min() < 0 or phi.max() >= Tb.shape[0]:
            raise ValueError(f"phi {phi.shape}: expected {k} indices into {Tb.shape[0]} states")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    paths = torch.empty(n_samples, N, dtype=torch.int32, device=dev)
    kw = {}
    if score is not None:
        kw = dict(Tb=torch.from_numpy(Tb).to(dev), Bb=torch.from_numpy(M.bridge_table(Tb, int(phi[end]), N)).to(dev), phi=phi,
                  prob=torch.empty(n_samples, dtype=torch.float64, device=dev))
    tp_sample_into(torch.from_numpy(Ta).to(dev), torch.from_numpy(Ba).to(dev), start, end, seed, stream, paths, sample_base, **kw)
    return (paths.cpu().numpy(), kw["prob"].cpu().numpy()) if score is not None else paths.cpu().numpy()


def analyze(traj_atom14, ref_atom14, aatype, nlag=NLAG, ref_nlag=None, pairs=DEFAULT_PAIRS, decorr=True, tica=False,
            tica_lag=TICA_LAG, msm=False, msm_k=KMEANS_K, msm_states=MSM_STATES, md_msm_lag=MD_MSM_LAG, msm_lag=MSM_LAG,
            traj_msm=True, kmeans_seed=KMEANS_SEED, name=None) -> dict:
    """The reference's per-peptide result for a sampled trajectory `traj_atom14` (F, L, 14, 3) against the MD trajectory
    `ref_atom14` (F_ref, L, 14, 3) -- a CUDA tensor, or an array that is copied to traj_atom14's device:

      "features"           the labels of `torsion_features(aatype)`
      "JSD"                {label: Jensen-Shannon distance of the two 100-bin histograms} and {"a|b": ... of the 50 x 50 ones} for
                           `pairs` of feature indices -- by default the reference's literal columns (1, 2) and (3, 4); pass
                           (phi_i, psi_i) index pairs for Ramachandran maps.  Pairs a short sequence does not have are dropped.
      "our_decorrelation"  {label: fp32 array [nlag + 1]} of `decorrelation` (nlag clamped to F - 1)
      "md_decorrelation"   the same of the MD trajectory, ref_nlag = min(100000, F_ref - 1) by default

    The last two only with `decorr`.  With `tica` (`tica_entries`: fitted on the MD trajectory at lag `tica_lag`), after these:
    JSD["TICA-0"] (100 bins over the two trajectories' common range of component 0) and JSD["TICA-0,1"] (50 x 50), with `decorr`
    our_decorrelation["tica"] / md_decorrelation["tica"], and

      "tica_model"         `TicaModel.as_dict()`: lag, mean, eigenvalues, W, dim, rank

    With `msm` (which implies `tica`; `msm_entries` on the projections at the model's `dim`, k-means with `msm_k` centres and
    `kmeans_seed`, PCCA+ into `msm_states` sets, the MD MSM at lag `md_msm_lag`, the sampled trajectory's at `msm_lag`), after these
    and in this order: "kmeans" {centers, dim, steps, cost, seed}, "msm", "pcca", "cmsm", "traj_metastable_probs",
    "ref_metastable_probs", "msm_transition_matrix", "pcca_pi", "msm_pi" and, unless `traj_msm` is False, "traj_msm",
    "traj_transition_matrix", "traj_pi" (left out, with `name` on stderr, when only the sampled trajectory's MSM cannot be
    estimated).  The estimators are the plain dicts of mdgen_amd/msm.py.

    ValueError when the MD trajectory has fewer than tica_lag + 2 frames, no torsions or more than 64, or a covariance of rank < 2;
    with `msm` also when it has fewer frames than centres, no pair of frames md_msm_lag apart, or a microstate outside the MSM's
    connected set.  Plain Python and NumPy objects only."""
    aat = _checked_aatype(aatype.cpu().numpy() if hasattr(aatype, "cpu") else aatype)
    traj = _device_f32(traj_atom14)
    ref = _device_f32(ref_atom14, traj.device)
    labels, _ = torsion_features(aat)
    NF = len(labels)
    tica = bool(tica or msm)
    if tica:   # (what tica_fit would refuse, before any launch)
        if int(tica_lag) < 0 or int(ref.shape[0]) - int(tica_lag) < 2:
            raise ValueError(f"tICA at lag {int(tica_lag)} needs at least lag + 2 frames, got {int(ref.shape[0])}")
        _check_tica_shape(int(ref.shape[0]), NF, int(tica_lag))
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
    if tica:
        t = tica_entries(a_traj, a_ref, tica_lag, nlag, ref_nlag, decorr, projections=bool(msm))
        out["JSD"]["TICA-0"], out["JSD"]["TICA-0,1"] = t["TICA-0"], t["TICA-0,1"]
        if decorr:
            out["our_decorrelation"]["tica"], out["md_decorrelation"]["tica"] = t["our_tica"], t["md_tica"]
        out["tica_model"] = t["model"]
        if msm:
            dim = t["model"]["dim"]      # (the reference's tica.transform has the model's dim columns)
            out.update(msm_entries(t["y_traj"][:, :dim].contiguous(), t["y_ref"][:, :dim].contiguous(), msm_k, msm_states,
                                   md_msm_lag, msm_lag, traj_msm, kmeans_seed, name))
    return out
