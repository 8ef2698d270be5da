"""Cartesian ensemble statistics of protein trajectories on the device: what an AlphaFlow-style ensemble evaluation is made of --
superposition on a reference structure, per-atom RMSF, mean pairwise RMSD within and between ensembles, the per-atom Gaussian
Wasserstein distance, contact-probability maps with weak and transient contacts, PCA of the C-alpha coordinates, and -- on request --
Shrake-Rupley solvent-accessible surface areas with the exposed-residue set and the mutual information of the exposure bits built
on them.  The kernels are csrc/k_ensemble.hip (`mdgen_ens_superpose`, `mdgen_ens_moments`, `mdgen_ens_pairwise_d2`,
`mdgen_ens_contact_counts`, `mdgen_ens_sasa_counts`, include/mdgen_amd.h); the 3 x 3 matrix square roots, the 3N x 3N
eigenproblem, the assignment problem and the L x L mutual-information table are NumPy / SciPy fp64 on the host.  Units are Angstrom.

Every quantity is defined by its equation in include/mdgen_amd.h and in the docstrings here.  AlphaFlow's evaluation script and
mdtraj are not installed where this was written: agreement with that script and with `mdtraj.superpose` / `mdtraj.rmsf` /
`mdtraj.shrake_rupley` is unverified (the surface defaults -- probe 2.8 A, side-chain area above 2.0 A^2 -- follow the AlphaFlow
paper's description); the yardstick is the NumPy restatement in tests/.  Out of scope: XTC output, plots, and a Gram-matrix form
of the pairwise distances.

`gaussian_w2`, `pca_w2`, `jaccard`, `contact_sets`, `sphere_points`, `atom_radii`, `mi_from_counts`, `spearman` and `exposed_sets`
import without torch; the functions on tensors import torch and the library
when they are called."""
from __future__ import annotations

import numpy as np

from .pdb import _checked_aatype, residue_tables

MAX_ATOMS = 16384               # include/mdgen_amd.h mdgen_ens_*: A
MAX_PAIR_FRAMES = (1 << 20) - 1   # mdgen_ens_pairwise_d2: Fa, Fb
MAX_RESIDUES = 4096             # mdgen_ens_contact_counts: N
MAX_FRAMES = 1 << 40
MAX_CONTACT_FRAMES = (1 << 31) - 1
MAX_PCA_DIM = 3072              # pca_fit: 3 N
WAVE_ATOMS = 256                # csrc/kernels.h kEnsWaveAtoms: up to here a wave owns a frame of mdgen_ens_superpose
PAIR_TILE_A = 128               # csrc/kernels.h kEnsPairTileA / B / Chunk: the tile of mdgen_ens_pairwise_d2
PAIR_TILE_B = 64
PAIR_CHUNK = 24
CONTACT_TILE = 64               # csrc/k_ensemble.hip kCcTile
CA_SLOT = 1                     # atom14 slot of the C-alpha
CUTOFF = 8.0                    # contact cutoff between C-alphas
WEAK_BELOW = 0.9
TRANSIENT_ABOVE = 0.1
MAX_SASA_POINTS = 4096          # csrc/kernels.h kEnsSasaMaxPoints: P of mdgen_ens_sasa_counts
MAX_SASA_RADIUS = 16.0          # kEnsSasaMaxRadius: every radius, and the probe
SASA_NEIGHBOURS = 512           # kEnsSasaMaxNeighbours: a wave's neighbour list; more within reach: every atom is tested
SASA_SCAN = 64                  # the atoms a wave scans at a time
SASA_COUNT_BYTES = 64 << 20     # the int32 counts of one call of `sasa_counts` / `residue_sasa`
BONDI_RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80}
SIDECHAIN_SLOT = 4              # atom14 slots 0 .. 3 are N, CA, C, O
SASA_PROBE = 2.8                # `analyze_ensemble`'s defaults: the probe radius, and the side-chain area (A^2) above which a
SASA_THRESHOLD = 2.0            # residue counts as exposed


# ---- shapes ----------------------------------------------------------------------------------------------------------
def _check_frames_atoms(F, A, min_atoms=1):
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"the number of frames must be in 1 .. 2^40, got {F}")
    if not min_atoms <= A <= MAX_ATOMS:
        raise ValueError(f"the number of atoms must be in {min_atoms} .. {MAX_ATOMS}, got {A}")


def _check_pairwise_shape(Fa, Fb, A):
    if not (1 <= Fa <= MAX_PAIR_FRAMES and 1 <= Fb <= MAX_PAIR_FRAMES):
        raise ValueError(f"pairwise distances take 1 .. {MAX_PAIR_FRAMES} frames a side, got {Fa} and {Fb}")
    if not 1 <= A <= MAX_ATOMS:
        raise ValueError(f"the number of atoms must be in 1 .. {MAX_ATOMS}, got {A}")


def _check_contact_shape(F, N, cutoff):
    if not 1 <= F <= MAX_CONTACT_FRAMES:
        raise ValueError(f"contact counts take 1 .. 2^31 - 1 frames, got {F}")
    if not 1 <= N <= MAX_RESIDUES:
        raise ValueError(f"contact counts take 1 .. {MAX_RESIDUES} residues, got {N}")
    if not (np.isfinite(cutoff) and cutoff >= 0):
        raise ValueError(f"the cutoff must be finite and >= 0, got {cutoff}")


def cutoff2_f32(cutoff) -> np.float32:
    """The squared cutoff the kernel compares with: squared in fp64, rounded to fp32 once."""
    return np.float32(np.float64(cutoff) * np.float64(cutoff))


def _coords(x, device=None):
    """(F, A, 3) fp32 contiguous device tensor of x [F, A, 3] or [F, L, 14, 3] (NumPy or torch)."""
    import torch
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.array(x, np.float32))   # (a copy: memory maps are read-only)
    if device is None and not x.is_cuda:
        from ._lib import MdgenError
        raise MdgenError("mdgen_amd.ensemble runs on the GPU only (no CPU fallback): got a CPU tensor")
    x = x.to(device=device if device is not None else x.device, dtype=torch.float32)
    if x.ndim == 4:
        x = x.reshape(x.shape[0], -1, 3)
    if x.ndim != 3 or x.shape[-1] != 3:
        raise ValueError(f"coordinates {tuple(x.shape)}: expected [F, A, 3] or [F, L, 14, 3]")
    return x.contiguous()


# ---- superposition ---------------------------------------------------------------------------------------------------
def superpose_into(x, ref, w, exists, out, rot=None, rmsd=None) -> None:
    """One `mdgen_ens_superpose` call on x's device and current stream: x (F, A, 3), ref (A, 3), w [A] fp32; exists uint8 [A] or
    None; out (F, A, 3) fp32 (may be x); rot fp64 (F, 9) and rmsd fp64 [F] or None.  The library copies w back and checks it:
    this call synchronises the stream once."""
    import torch
    from ._lib import launch, lib, ptr
    F, A = int(x.shape[0]), int(x.shape[1])
    _check_frames_atoms(F, A, 3)
    f32 = torch.float32
    if ref.numel() != A * 3 or w.numel() != A or out.numel() != F * A * 3 or (exists is not None and exists.numel() != A):
        raise ValueError("ref must be [A, 3], w and exists [A], out [F, A, 3]")
    if (rot is not None and rot.numel() < F * 9) or (rmsd is not None and rmsd.numel() < F):
        raise ValueError("rot needs F * 9 elements, rmsd F")
    launch(lib.mdgen_ens_superpose, x, F, A, ptr(x, f32), ptr(ref, f32), ptr(w, f32), ptr(exists, torch.uint8), ptr(out, f32),
           ptr(rot, torch.float64), ptr(rmsd, torch.float64))


def superpose(x, ref, weights=None, exists=None, out=None, with_rot=False, with_rmsd=False):
    """x (F, A, 3) (or (F, L, 14, 3)) superposed on ref (A, 3) under `weights` [A] (default: 1 where `exists`, else everywhere):
    a new device tensor of x's shape, or `out` (which may be x).  Atoms with exists == 0 are copied unchanged.  With `with_rot` /
    `with_rmsd` a tuple (out[, rot fp64 (F, 3, 3)][, rmsd fp64 (F,)]) of device tensors."""
    import torch
    shape = tuple(x.shape) if hasattr(x, "shape") else None
    xd = _coords(x)
    dev = xd.device
    F, A = int(xd.shape[0]), int(xd.shape[1])
    if not torch.is_tensor(ref):
        ref = torch.from_numpy(np.array(ref, np.float32))
    refd = ref.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    ex = None
    if exists is not None:
        ex = (torch.as_tensor(exists).reshape(-1) != 0).to(device=dev, dtype=torch.uint8)
    if weights is None:
        w = ex.to(torch.float32) if ex is not None else torch.ones(A, dtype=torch.float32, device=dev)
    else:
        w = torch.as_tensor(weights, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    if out is None:
        o = torch.empty_like(xd)
    else:
        o = out.reshape(F, A, 3)
        if o.data_ptr() != out.data_ptr():
            raise ValueError("out must be contiguous")
    rot = torch.empty(F, 9, dtype=torch.float64, device=dev) if with_rot else None
    rmsd = torch.empty(F, dtype=torch.float64, device=dev) if with_rmsd else None
    superpose_into(xd, refd, w, ex, o, rot, rmsd)
    res = o.reshape(shape) if out is None else out
    if not (with_rot or with_rmsd):
        return res
    return (res,) + ((rot.reshape(F, 3, 3),) if with_rot else ()) + ((rmsd,) if with_rmsd else ())


# ---- moments ---------------------------------------------------------------------------------------------------------
def moments_workspace_bytes(F, A) -> int:
    import ctypes
    from ._lib import check, lib
    _check_frames_atoms(int(F), int(A))
    n = ctypes.c_size_t()
    check(lib.mdgen_ens_moments_workspace_bytes(int(F), int(A), ctypes.byref(n)))
    return int(n.value)


def moments_into(x, mean, cov, workspace) -> None:
    """One `mdgen_ens_moments` call: x (F, A, 3) fp32; mean fp64 [A, 3] and cov fp64 [A, 3, 3] written."""
    import torch
    from ._lib import launch, lib, ptr
    F, A = int(x.shape[0]), int(x.shape[1])
    _check_frames_atoms(F, A)
    if mean.numel() < A * 3 or cov.numel() < A * 9:
        raise ValueError("mean needs A * 3 elements, cov A * 9")
    launch(lib.mdgen_ens_moments, x, F, A, ptr(x, torch.float32), ptr(mean, torch.float64), ptr(cov, torch.float64),
           ptr(workspace, torch.uint8), int(workspace.numel()))


def moments_device(x):
    """(mean fp64 [A, 3], cov fp64 [A, 3, 3]) of every atom over the frames of x (F, A, 3), as device tensors."""
    import torch
    x = _coords(x)
    F, A = int(x.shape[0]), int(x.shape[1])
    mean = torch.empty(A, 3, dtype=torch.float64, device=x.device)
    cov = torch.empty(A, 3, 3, dtype=torch.float64, device=x.device)
    ws = torch.empty(max(moments_workspace_bytes(F, A), 16), dtype=torch.uint8, device=x.device)
    moments_into(x, mean, cov, ws)
    return mean, cov


def moments(x):
    """(mean [A, 3], cov [A, 3, 3]) as NumPy fp64: the per-atom mean and covariance over the frames, divided by F."""
    mean, cov = moments_device(x)
    return mean.cpu().numpy(), cov.cpu().numpy()


def rmsf(x) -> np.ndarray:
    """Per-atom root-mean-square fluctuation about the mean position, sqrt(trace cov), fp64 [A]: x is taken as it is (superpose
    it first)."""
    cov = moments(x)[1]
    return np.sqrt(np.maximum(np.trace(cov, axis1=1, axis2=2), 0.0))


# ---- pairwise RMSD ---------------------------------------------------------------------------------------------------
def pairwise_workspace_bytes(Fa, Fb, A) -> int:
    import ctypes
    from ._lib import check, lib
    _check_pairwise_shape(int(Fa), int(Fb), int(A))
    n = ctypes.c_size_t()
    check(lib.mdgen_ens_pairwise_d2_workspace_bytes(int(Fa), int(Fb), int(A), ctypes.byref(n)))
    return int(n.value)


def pairwise_d2_into(xa, xb, d2, sums, workspace) -> None:
    """One `mdgen_ens_pairwise_d2` call: xa (Fa, A, 3), xb (Fb, A, 3) fp32 (may be one tensor); d2 fp32 [Fa, Fb] or None; sums
    fp64 [2] = (sum of sqrt(d2 / A), sum of d2 / A) over all pairs."""
    import torch
    from ._lib import launch, lib, ptr
    Fa, Fb, A = int(xa.shape[0]), int(xb.shape[0]), int(xa.shape[1])
    _check_pairwise_shape(Fa, Fb, A)
    if int(xb.shape[1]) != A:
        raise ValueError(f"the ensembles have {A} and {int(xb.shape[1])} atoms")
    if (d2 is not None and d2.numel() < Fa * Fb) or sums.numel() < 2:
        raise ValueError("d2 needs Fa * Fb elements, sums 2")
    launch(lib.mdgen_ens_pairwise_d2, xa, Fa, Fb, A, ptr(xa, torch.float32), ptr(xb, torch.float32), ptr(d2, torch.float32),
           ptr(sums, torch.float64), ptr(workspace, torch.uint8), int(workspace.numel()))


def pairwise_rmsd(xa, xb=None, matrix=False):
    """(mean, rms) of the RMSD sqrt(sum (xa_i - xb_j)^2 / A) over all pairs of frames, without superposing the pairs (superpose
    the ensembles on one structure first): mean = sum sqrt(d2 / A) / (Fa Fb), rms = sqrt(sum (d2 / A) / (Fa Fb)).  xb None: xa
    against itself, the zero diagonal included.  With `matrix` also the fp32 device tensor [Fa, Fb] of sqrt(d2 / A)."""
    import torch
    xa = _coords(xa)
    xb = xa if xb is None else _coords(xb, xa.device)
    Fa, Fb, A = int(xa.shape[0]), int(xb.shape[0]), int(xa.shape[1])
    d2 = torch.empty(Fa, Fb, dtype=torch.float32, device=xa.device) if matrix else None
    sums = torch.empty(2, dtype=torch.float64, device=xa.device)
    ws = torch.empty(max(pairwise_workspace_bytes(Fa, Fb, A), 16), dtype=torch.uint8, device=xa.device)
    pairwise_d2_into(xa, xb, d2, sums, ws)
    s = sums.cpu().numpy()
    mean, rms = float(s[0] / (Fa * Fb)), float(np.sqrt(s[1] / (Fa * Fb)))
    return (mean, rms, torch.sqrt(d2 / A)) if matrix else (mean, rms)


# ---- contacts --------------------------------------------------------------------------------------------------------
def contact_counts_into(ca, cutoff, counts) -> None:
    """One `mdgen_ens_contact_counts` call: ca (F, N, 3) fp32; counts int32 [N, N] zeroed and filled."""
    import torch
    from ._lib import launch, lib, ptr
    F, N = int(ca.shape[0]), int(ca.shape[1])
    _check_contact_shape(F, N, cutoff)
    if counts.numel() < N * N:
        raise ValueError("counts needs N * N elements")
    launch(lib.mdgen_ens_contact_counts, ca, F, N, ptr(ca, torch.float32), float(cutoff2_f32(cutoff)), ptr(counts, torch.int32))


def contact_counts(ca, cutoff=CUTOFF) -> np.ndarray:
    """counts int32 [N, N] (NumPy): the number of frames of ca (F, N, 3) in which residues i and j are closer than `cutoff`
    (squared distance in fp32 against the cutoff squared in fp64 and rounded to fp32 once)."""
    import torch
    ca = _coords(ca)
    counts = torch.empty(int(ca.shape[1]), int(ca.shape[1]), dtype=torch.int32, device=ca.device)
    contact_counts_into(ca, cutoff, counts)
    return counts.cpu().numpy()


# ---- solvent-accessible surface --------------------------------------------------------------------------------------
def _check_sasa_shape(F, A, P, probe):
    if not 1 <= F <= MAX_CONTACT_FRAMES:
        raise ValueError(f"surface counts take 1 .. 2^31 - 1 frames, got {F}")
    if not 1 <= A <= MAX_ATOMS:
        raise ValueError(f"the number of atoms must be in 1 .. {MAX_ATOMS}, got {A}")
    if not 1 <= P <= MAX_SASA_POINTS:
        raise ValueError(f"the number of sphere points must be in 1 .. {MAX_SASA_POINTS}, got {P}")
    if not (np.isfinite(probe) and 0 <= probe <= MAX_SASA_RADIUS):
        raise ValueError(f"the probe radius must be in 0 .. {MAX_SASA_RADIUS:g}, got {probe}")


def sphere_points(n) -> np.ndarray:
    """fp32 [n, 3]: the golden-section spiral on the unit sphere, computed in fp64 and rounded to fp32 once.
    y_i = (2 i + 1) / n - 1, r_i = sqrt(1 - y_i^2), phi_i = i pi (3 - sqrt 5); point (cos phi_i r_i, y_i, sin phi_i r_i)."""
    n = int(n)
    if not 1 <= n <= MAX_SASA_POINTS:
        raise ValueError(f"the number of sphere points must be in 1 .. {MAX_SASA_POINTS}, got {n}")
    i = np.arange(n, dtype=np.float64)
    y = (2.0 * i + 1.0) / n - 1.0
    r = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], -1).astype(np.float32)


def atom_radii(aatype) -> np.ndarray:
    """fp32 [14 L]: the Bondi radius of every atom14 slot of a sequence by its element -- the first letter of the atom's name,
    `atom_types[atom14_to_atom37]` -- C 1.70, N 1.55, O 1.52, S 1.80 A; 0 where `atom14_mask` is 0 (no atom)."""
    t = residue_tables()
    aatype = _checked_aatype(aatype)
    names = np.asarray(t["atom_types"])[np.asarray(t["atom14_to_atom37"])[aatype]]          # [L, 14]
    mask = np.asarray(t["atom14_mask"])[aatype] != 0
    rad = np.zeros(names.shape, np.float32)
    for slot in np.argwhere(mask):
        rad[tuple(slot)] = BONDI_RADII[str(names[tuple(slot)])[0]]
    return rad.reshape(-1)


def sasa_workspace_bytes(A, P) -> int:
    import ctypes
    from ._lib import check, lib
    _check_sasa_shape(1, int(A), int(P), 0.0)
    n = ctypes.c_size_t()
    check(lib.mdgen_ens_sasa_workspace_bytes(int(A), int(P), ctypes.byref(n)))
    return int(n.value)


def _host_f32(a, shape, what):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    if a.shape != shape:
        raise ValueError(f"{what} must have shape {shape}, got {a.shape}")
    return a


def sasa_counts_into(x, radius, points, probe, counts, workspace) -> None:
    """One `mdgen_ens_sasa_counts` call: x (F, A, 3) fp32 on the device; radius [A] and points [P, 3] HOST arrays (NumPy); counts
    int32 with F * A elements, every one written; workspace: `sasa_workspace_bytes(A, P)` bytes of uint8 on the device."""
    import torch
    from ._lib import launch, lib, ptr
    F, A = int(x.shape[0]), int(x.shape[1])
    points = np.asarray(points, np.float32)
    P = int(points.shape[0]) if points.ndim == 2 else 0
    _check_sasa_shape(F, A, P, probe)
    radius, points = _host_f32(radius, (A,), "radius"), _host_f32(points, (P, 3), "points")
    if counts.numel() < F * A:
        raise ValueError("counts needs F * A elements")
    launch(lib.mdgen_ens_sasa_counts, x, F, A, P, ptr(x, torch.float32), radius.ctypes.data, points.ctypes.data, float(probe),
           ptr(counts, torch.int32), ptr(workspace, torch.uint8), int(workspace.numel()))


def _sasa_chunk(A, chunk=None):
    """Frames of one call: what `chunk` says, else as many as keep the call's int32 counts within SASA_COUNT_BYTES."""
    return max(1, SASA_COUNT_BYTES // (4 * int(A))) if chunk is None else max(1, int(chunk))


def sasa_counts(x, radius, n_points=960, probe=1.4, chunk=None):
    """counts int32 [F, A], a device tensor: the number of the `n_points` points of `sphere_points` on the sphere of radius
    radius[a] + probe about atom a of frame f that no other atom buries (include/mdgen_amd.h `mdgen_ens_sasa_counts`); 0 where
    radius[a] == 0.  The area is 4 pi (radius + probe)^2 counts / n_points.  One call per `chunk` frames (default: 64 MB of counts
    a call); a frame's counts do not depend on the chunk it falls in."""
    import torch
    x = _coords(x)
    F, A = int(x.shape[0]), int(x.shape[1])
    points = sphere_points(n_points)
    _check_sasa_shape(F, A, len(points), probe)
    counts = torch.empty(F, A, dtype=torch.int32, device=x.device)
    ws = torch.empty(sasa_workspace_bytes(A, len(points)), dtype=torch.uint8, device=x.device)
    step = _sasa_chunk(A, chunk)
    for f0 in range(0, F, step):
        sasa_counts_into(x[f0:f0 + step], radius, points, probe, counts[f0:f0 + step], ws)
    return counts


def sasa_areas(radius, probe, n_points, select=None) -> np.ndarray:
    """fp64 [A]: the area 4 pi R_a^2 / n_points of one point of atom a, R_a = radius[a] + probe the fp32 sum taken to fp64; 0 where
    there is no atom (radius 0) or `select` [A] is False."""
    radius = np.asarray(radius, np.float32)
    R = np.where(radius != 0, radius + np.float32(probe), np.float32(0)).astype(np.float32).astype(np.float64)
    area = 4.0 * np.pi * R * R / int(n_points)
    return area if select is None else np.where(np.asarray(select, bool), area, 0.0)


def residue_sasa(atom14, aatype, atoms="sidechain", probe=2.8, n_points=960):
    """fp64 [F, L], a device tensor: the solvent-accessible area (A^2) of every residue of atom14 (F, L, 14, 3) in every frame --
    `sasa_counts` over all existing atoms with `atom_radii`, then the areas 4 pi R_a^2 counts / n_points of the residue's selected
    atoms added: atoms "sidechain" the atom14 slots >= 4 (glycine has none: area 0), "all" every existing atom.  Frame chunks of at
    most 64 MB of counts: no [F, 14 L] array exists."""
    import torch
    if atoms not in ("sidechain", "all"):
        raise ValueError(f"atoms must be 'sidechain' or 'all', got {atoms!r}")
    aatype = _checked_aatype(aatype)
    L = int(aatype.shape[0])
    x = _coords(atom14)
    F, A = int(x.shape[0]), int(x.shape[1])
    if A != 14 * L:
        raise ValueError(f"{L} residues need {14 * L} atom14 slots, got {A}")
    radius, points = atom_radii(aatype), sphere_points(n_points)
    _check_sasa_shape(F, A, len(points), probe)
    select = np.tile(np.arange(14) >= (SIDECHAIN_SLOT if atoms == "sidechain" else 0), L)
    m = np.zeros((A, L))
    m[np.arange(A), np.arange(A) // 14] = sasa_areas(radius, probe, len(points), select)
    m = torch.from_numpy(m).to(x.device)
    step = _sasa_chunk(A)
    counts = torch.empty(min(step, F), A, dtype=torch.int32, device=x.device)
    ws = torch.empty(sasa_workspace_bytes(A, len(points)), dtype=torch.uint8, device=x.device)
    out = torch.empty(F, L, dtype=torch.float64, device=x.device)
    for f0 in range(0, F, step):
        n = min(step, F - f0)
        sasa_counts_into(x[f0:f0 + n], radius, points, probe, counts[:n], ws)
        out[f0:f0 + n] = counts[:n].double() @ m
    return out


def exposure_mi(exposed, chunk=65536) -> np.ndarray:
    """fp64 [L, L] (NumPy), in nats: the mutual information of the exposure bits of every pair of residues over the frames of
    `exposed`, bool [F, L] (a torch tensor on any device, or NumPy: then on the host).  n_i = sum_t e_ti and n11 = E^T E are
    formed where the tensor is, in chunks of frames, as fp64 matmuls (exact: integers below 2^53); the four joint probabilities
    are p11 = n11 / F, p10 = (n_i - n11) / F, p01 = (n_j - n11) / F, p00 = 1 - p11 - p10 - p01 from the integers;
    MI = sum_ab p_ab ln(p_ab / (p_a p_b)), a term with p_ab = 0 being 0.  The diagonal is the entropy of e_i."""
    if isinstance(exposed, np.ndarray):
        e = exposed.astype(bool)
        F, L = e.shape
        n11 = np.zeros((L, L))
        for f0 in range(0, F, int(chunk)):
            y = e[f0:f0 + int(chunk)].astype(np.float64)
            n11 += y.T @ y
    else:
        import torch
        F, L = int(exposed.shape[0]), int(exposed.shape[1])
        acc = torch.zeros(L, L, dtype=torch.float64, device=exposed.device)
        for f0 in range(0, F, int(chunk)):
            y = (exposed[f0:f0 + int(chunk)] != 0).double()
            acc += y.T @ y
        n11 = acc.cpu().numpy()
    return mi_from_counts(n11, F)


def mi_from_counts(n11, F) -> np.ndarray:
    """`exposure_mi` from n11 = E^T E [L, L] (its diagonal is n_i) and the number of frames."""
    n11 = np.rint(np.asarray(n11, np.float64))
    n = np.diag(n11).copy()
    cells = ((n11, n[:, None], n[None, :]),                                  # (joint count, count of a, count of b)
             (n[:, None] - n11, n[:, None], F - n[None, :]),
             (n[None, :] - n11, F - n[:, None], n[None, :]),
             (F - n[:, None] - n[None, :] + n11, F - n[:, None], F - n[None, :]))
    mi = np.zeros_like(n11)
    for nab, na, nb in cells:
        nab, na, nb = np.broadcast_arrays(nab, na, nb)
        live = nab > 0
        pab = nab[live] / F
        mi[live] += pab * np.log(pab / ((na[live] / F) * (nb[live] / F)))
    return mi


def spearman(a, b) -> float:
    """Spearman's rank correlation: `pearson` of the average ranks (ties share the mean of their ranks); NaN when either side is
    constant."""
    def ranks(v):
        _, inverse, count = np.unique(np.asarray(v, np.float64).ravel(), return_inverse=True, return_counts=True)
        return (np.cumsum(count) - (count - 1) / 2.0)[inverse]
    return pearson(ranks(a), ranks(b))


def exposed_sets(prob, exposed_in_ref) -> np.ndarray:
    """bool [L]: the residues that are not exposed in the reference structure and whose exposure probability is > 0.1 -- the
    *transient* rule of `contact_sets`."""
    return ~np.asarray(exposed_in_ref, bool) & (np.asarray(prob, np.float64) > TRANSIENT_ABOVE)


# ---- host side: NumPy fp64 -------------------------------------------------------------------------------------------
def _sqrtm_psd(m):
    """Square roots of symmetric positive semi-definite matrices [..., 3, 3] by eigh; tiny negative eigenvalues clipped to 0."""
    lam, v = np.linalg.eigh(m)
    return (v * np.sqrt(np.maximum(lam, 0.0))[..., None, :]) @ np.swapaxes(v, -1, -2)


def gaussian_w2(mean_a, cov_a, mean_b, cov_b):
    """The squared 2-Wasserstein distance between the per-atom Gaussians N(mean_a, cov_a) and N(mean_b, cov_b):
    |mu_a - mu_b|^2 + tr(S_a + S_b - 2 (S_a^1/2 S_b S_a^1/2)^1/2), by symmetric eigh.  Returns (translation part [A], variance
    part [A] (clipped at 0), sqrt of the mean over the atoms of their sum)."""
    mean_a, mean_b = np.asarray(mean_a, np.float64), np.asarray(mean_b, np.float64)
    cov_a, cov_b = np.asarray(cov_a, np.float64), np.asarray(cov_b, np.float64)
    trans = ((mean_a - mean_b) ** 2).sum(-1)
    ra = _sqrtm_psd(cov_a)
    inner = ra @ cov_b @ ra
    inner = 0.5 * (inner + np.swapaxes(inner, -1, -2))
    cross = np.sqrt(np.maximum(np.linalg.eigvalsh(inner), 0.0)).sum(-1)
    var = np.maximum(np.trace(cov_a, axis1=-2, axis2=-1) + np.trace(cov_b, axis1=-2, axis2=-1) - 2.0 * cross, 0.0)
    return trans, var, float(np.sqrt(np.mean(trans + var)))


def pca_fit(ca, chunk=4096) -> dict:
    """PCA of the flattened coordinates of ca (F, N, 3), 3 N <= 3072: the mean from `moments`, the 3N x 3N covariance (divided by F)
    as a chunked fp64 matmul on the device, `eigh` on the host.  {"mean" [3N], "components" [3N, 3N] (rows, eigenvalues
    descending, each row's largest-magnitude entry positive), "eigenvalues" [3N], "explained" [3N]}."""
    import torch
    ca = _coords(ca)
    F, D = int(ca.shape[0]), int(ca.shape[1]) * 3
    if D > MAX_PCA_DIM:
        raise ValueError(f"PCA takes at most {MAX_PCA_DIM} coordinates, got {D}")
    mean = moments_device(ca)[0].reshape(1, D)
    c = torch.zeros(D, D, dtype=torch.float64, device=ca.device)
    flat = ca.reshape(F, D)
    for i in range(0, F, int(chunk)):
        y = flat[i:i + int(chunk)].double() - mean
        c += y.T @ y
    c = (c / F).cpu().numpy()
    lam, v = np.linalg.eigh(0.5 * (c + c.T))
    lam, comp = lam[::-1].copy(), v[:, ::-1].T.copy()
    big = np.abs(comp).argmax(1)
    comp *= np.sign(comp[np.arange(D), big])[:, None]
    total = lam.sum()
    return {"mean": mean.cpu().numpy().reshape(D), "components": comp, "eigenvalues": lam,
            "explained": lam / total if total > 0 else np.zeros_like(lam)}


def pca_project(ca, fit, k=2) -> np.ndarray:
    """(F, k) fp64: the frames of ca (F, N, 3) on the first k components of `fit` (a device matmul in fp64)."""
    import torch
    ca = _coords(ca)
    F = int(ca.shape[0])
    mean = torch.from_numpy(fit["mean"]).to(ca.device)
    comp = torch.from_numpy(np.ascontiguousarray(fit["components"][:k])).to(ca.device)
    return ((ca.reshape(F, -1).double() - mean) @ comp.T).cpu().numpy()


def pca_w2(proj_a, proj_b) -> float:
    """This project's definition of the 2-Wasserstein distance between two projected ensembles: ensemble a against len(a) frames
    of b taken at np.round(np.linspace(0, Fb - 1, Fa)), sqrt of the mean squared distance under the optimal one-to-one assignment
    (scipy.optimize.linear_sum_assignment)."""
    from scipy.optimize import linear_sum_assignment
    a, b = np.asarray(proj_a, np.float64), np.asarray(proj_b, np.float64)
    b = b[np.round(np.linspace(0, len(b) - 1, len(a))).astype(np.int64)]
    cost = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    r, c = linear_sum_assignment(cost)
    return float(np.sqrt(cost[r, c].mean()))


def jaccard(a, b) -> float:
    """|a and b| / |a or b| of two boolean arrays; NaN for an empty union."""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    union = int((a | b).sum())
    return float((a & b).sum() / union) if union else float("nan")


def contact_sets(prob, in_ref):
    """(weak, transient) boolean [N, N] over the pairs i < j: weak = in contact in the reference structure with probability
    < 0.9; transient = not in contact there with probability > 0.1."""
    prob, in_ref = np.asarray(prob, np.float64), np.asarray(in_ref, bool)
    upper = np.triu(np.ones(prob.shape, bool), 1)
    return upper & in_ref & (prob < WEAK_BELOW), upper & ~in_ref & (prob > TRANSIENT_ABOVE)


def pearson(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a - a.mean(), b - b.mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return float((a * b).sum() / den) if den > 0 else float("nan")


def fit_weights(aatype, fit="heavy"):
    """(weights fp32 [14 L], exists uint8 [14 L]) of a sequence: the existing atoms are `atom14_mask[aatype]`; fit "heavy" weighs
    every one of them 1, fit "ca" the C-alphas alone."""
    if fit not in ("heavy", "ca"):
        raise ValueError(f"fit must be 'heavy' or 'ca', got {fit!r}")
    mask = np.asarray(residue_tables()["atom14_mask"])[_checked_aatype(aatype)] != 0      # [L, 14]
    w = mask.astype(np.float32)
    if fit == "ca":
        w = np.zeros_like(w)
        w[:, CA_SLOT] = 1.0
    return w.reshape(-1), mask.astype(np.uint8).reshape(-1)


def superpose_on_first(atom14, aatype):
    """A trajectory (F, L, 14, 3), a device tensor, superposed on its own first frame over its existing atoms, unweighted: the
    reference's `traj.superpose(traj)`.  A new tensor."""
    import torch
    w, ex = fit_weights(aatype, "heavy")
    first = atom14[0].clone()
    return superpose(atom14, first, weights=torch.from_numpy(w), exists=ex)


def analyze_ensemble(traj_atom14, ref_atom14, aatype, fit="heavy", cutoff=CUTOFF, pca=True, sasa=False, probe=SASA_PROBE, n_points=960,
                     sasa_threshold=SASA_THRESHOLD, sasa_atoms="sidechain") -> dict:
    """The ensemble statistics of a sampled trajectory (T, L, 14, 3) against an MD ensemble (F, L, 14, 3), both superposed on frame 0
    of the MD ensemble over the existing heavy atoms (`fit="heavy"`) or the C-alphas (`fit="ca"`).  Plain NumPy arrays and floats:
      ca_rmsf, ref_ca_rmsf [L]; atom_rmsf, ref_atom_rmsf [L, 14] (0 where no atom); rmsf_pearson (of the C-alpha RMSFs);
      mean_pairwise_rmsd, ref_mean_pairwise_rmsd, cross_mean_pairwise_rmsd and rms_pairwise_rmsd, ref_rms_..., cross_rms_...
        (`pairwise_rmsd` over the C-alphas: sampled x sampled, MD x MD, sampled x MD);
      emd_mean, emd_var, emd_total: `gaussian_w2` over the C-alphas -- sqrt of the mean translation part, of the mean variance
        part, and of the mean of their sum;
      contact_prob, ref_contact_prob [L, L]: `contact_counts` / frames;
      weak_contacts_jaccard, transient_contacts_jaccard: `contact_sets` of the MD and of the sampled probabilities, both against
        the contacts of the reference structure (frame 0 of the MD ensemble), compared by `jaccard`;
      with `pca`: pca_w2_ref (both ensembles on the MD ensemble's first two components), pca_w2_joint (on those of the two
        ensembles stacked, MD first), pca_explained [2] (of the MD ensemble's);
      with `sasa`, after those (`residue_sasa` of the superposed coordinates with `probe`, `n_points`, `sasa_atoms`):
        residue_sasa_mean, ref_residue_sasa_mean [L] (A^2, over the frames);
        exposure_prob, ref_exposure_prob [L]: the share of frames in which the residue's area is > `sasa_threshold`;
        exposed_residue_jaccard: `exposed_sets` -- the residues not exposed in the reference structure (frame 0 of the MD
          ensemble) with exposure probability > 0.1 -- of the MD and of the sampled probabilities, compared by `jaccard`;
        exposed_mi, ref_exposed_mi [L, L]: `exposure_mi` of the exposure bits (nats);
        exposed_mi_spearman: `spearman` of the two matrices over the pairs i < j."""
    import torch
    aatype = _checked_aatype(aatype)
    L = int(aatype.shape[0])
    x = _coords(traj_atom14, None if torch.is_tensor(traj_atom14) and traj_atom14.is_cuda else torch.device("cuda"))
    r = _coords(ref_atom14, x.device)
    if int(x.shape[1]) != 14 * L or int(r.shape[1]) != 14 * L:
        raise ValueError(f"{L} residues need {14 * L} atom14 slots, got {int(x.shape[1])} and {int(r.shape[1])}")
    w, ex = fit_weights(aatype, fit)
    target = r[0].clone()
    x = superpose(x, target, weights=w, exists=ex)
    r = superpose(r, target, weights=w, exists=ex)
    out = {}
    mx, cx = moments(x)
    mr, cr = moments(r)
    exists = ex.reshape(L, 14) != 0
    for key, c in (("atom_rmsf", cx), ("ref_atom_rmsf", cr)):
        out[key] = np.where(exists, np.sqrt(np.maximum(np.trace(c, axis1=1, axis2=2), 0.0)).reshape(L, 14), 0.0)
    out["ca_rmsf"], out["ref_ca_rmsf"] = out["atom_rmsf"][:, CA_SLOT].copy(), out["ref_atom_rmsf"][:, CA_SLOT].copy()
    out["rmsf_pearson"] = pearson(out["ca_rmsf"], out["ref_ca_rmsf"])
    ca_x = x.reshape(-1, L, 14, 3)[:, :, CA_SLOT].contiguous()
    ca_r = r.reshape(-1, L, 14, 3)[:, :, CA_SLOT].contiguous()
    for pre, a, b in (("", ca_x, None), ("ref_", ca_r, None), ("cross_", ca_x, ca_r)):
        out[pre + "mean_pairwise_rmsd"], out[pre + "rms_pairwise_rmsd"] = pairwise_rmsd(a, b)
    sel = np.arange(L) * 14 + CA_SLOT
    trans, var, total = gaussian_w2(mx[sel], cx[sel], mr[sel], cr[sel])
    out["emd_mean"], out["emd_var"], out["emd_total"] = float(np.sqrt(trans.mean())), float(np.sqrt(var.mean())), total
    out["contact_prob"] = contact_counts(ca_x, cutoff) / float(ca_x.shape[0])
    out["ref_contact_prob"] = contact_counts(ca_r, cutoff) / float(ca_r.shape[0])
    in_ref = contact_counts(ca_r[:1], cutoff) > 0
    weak_r, trans_r = contact_sets(out["ref_contact_prob"], in_ref)
    weak_x, trans_x = contact_sets(out["contact_prob"], in_ref)
    out["weak_contacts_jaccard"], out["transient_contacts_jaccard"] = jaccard(weak_r, weak_x), jaccard(trans_r, trans_x)
    if pca:
        fit_r = pca_fit(ca_r)
        out["pca_w2_ref"] = pca_w2(pca_project(ca_x, fit_r), pca_project(ca_r, fit_r))
        fit_j = pca_fit(torch.cat([ca_r, ca_x], 0))
        out["pca_w2_joint"] = pca_w2(pca_project(ca_x, fit_j), pca_project(ca_r, fit_j))
        out["pca_explained"] = fit_r["explained"][:2].copy()
    if sasa:
        if not np.isfinite(sasa_threshold):
            raise ValueError(f"sasa_threshold must be finite, got {sasa_threshold}")
        bits, prob = {}, {}
        for pre, coords in (("", x), ("ref_", r)):
            area = residue_sasa(coords, aatype, atoms=sasa_atoms, probe=probe, n_points=n_points)     # [frames, L] fp64, on the device
            bits[pre] = area > float(sasa_threshold)
            out[pre + "residue_sasa_mean"] = area.mean(0).cpu().numpy()
            prob[pre] = bits[pre].sum(0).cpu().numpy() / float(area.shape[0])
        out["exposure_prob"], out["ref_exposure_prob"] = prob[""], prob["ref_"]
        in_ref = bits["ref_"][0].cpu().numpy()
        out["exposed_residue_jaccard"] = jaccard(exposed_sets(out["ref_exposure_prob"], in_ref),
                                                 exposed_sets(out["exposure_prob"], in_ref))
        out["exposed_mi"], out["ref_exposed_mi"] = exposure_mi(bits[""]), exposure_mi(bits["ref_"])
        upper = np.triu_indices(L, 1)
        out["exposed_mi_spearman"] = spearman(out["exposed_mi"][upper], out["ref_exposed_mi"][upper])
    return out
