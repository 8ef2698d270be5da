"""mdgen_amd.analysis restated in NumPy fp64, and the cases its tests share.

The restatement is what the kernels of csrc/k_analysis.hip are held against (tests/test_analysis_gpu.py) and is itself held
against independent evaluations on the CPU (tests/test_analysis_cpu.py): np.histogram / np.histogram2d, a double loop for the
autocovariance, scipy's jensenshannon, hand-built dihedrals.

Gates.  Dihedrals: the wrapped difference |((a - b + pi) mod 2 pi) - pi| to the fp64 angle of the same fp32 coordinates, at most
max(32 x floor, eps32), floor = the largest such difference of the same formula in torch fp32 on the CPU over the case's compared
quadruples.  Compared are quadruples with |b2 x b3| and |b1 x b2| above 1e-3 A^2 in fp64; at most 1 % of a case may fall below
(`dihedral_case` asserts it), the others only have to be finite.  Autocovariance: absolute difference to the fp64 FFT evaluation
(own error about 1e-13), at most max(32 x floor, eps32), floor = the largest error over the lags of np.dot in fp32 on the fp32
sin / cos of the series.  Histograms are exact."""
import functools

import numpy as np

from mdgen_amd.analysis import BINS_1D, BINS_2D, DEFAULT_PAIRS, MD_NLAG, NLAG, hist_edges, jsd, torsion_features

EPS32 = float(np.finfo(np.float32).eps)
ILL = 1e-3          # A^2: a cross product below this makes the angle ill-conditioned
PI32 = np.float32(np.pi)


# ---- the algorithms -------------------------------------------------------------------------------------------------
def dihedral_parts(atom14, quad):
    """fp64: (angles [F, NF], well [F, NF] bool) of atom14 [F, L, 14, 3] for the index table quad [NF, 4]."""
    a = np.asarray(atom14, np.float64).reshape(atom14.shape[0], -1, 3)
    p = a[:, np.asarray(quad, np.int64).reshape(-1, 4)]                       # [F, NF, 4, 3]
    b1, b2, b3 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1], p[:, :, 3] - p[:, :, 2]
    c1, c2 = np.cross(b2, b3), np.cross(b1, b2)
    y = np.linalg.norm(b2, axis=-1) * (b1 * c1).sum(-1)
    x = (c1 * c2).sum(-1)
    well = (np.linalg.norm(c1, axis=-1) > ILL) & (np.linalg.norm(c2, axis=-1) > ILL)
    return np.arctan2(y, x), well


def dihedrals(atom14, quad):
    return dihedral_parts(atom14, quad)[0]


def dihedrals_torch32(atom14, quad):
    """The same formula in torch fp32 on the CPU: the floor of the dihedral gate."""
    import torch
    a = torch.from_numpy(np.ascontiguousarray(atom14, np.float32)).reshape(atom14.shape[0], -1, 3)
    p = a[:, torch.from_numpy(np.asarray(quad, np.int64).reshape(-1, 4))]
    b1, b2, b3 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1], p[:, :, 3] - p[:, :, 2]
    c1, c2 = torch.linalg.cross(b2, b3), torch.linalg.cross(b1, b2)
    y = b2.norm(dim=-1) * (b1 * c1).sum(-1)
    x = (c1 * c2).sum(-1)
    assert y.dtype == torch.float32
    return torch.atan2(y, x).numpy()


def wrapped(a, b):
    return np.abs(np.mod(np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi, 2 * np.pi) - np.pi)


def bins_of(x, edges):
    """searchsorted(edges, x, 'right') - 1, the last edge in the last bin, -1 outside [edges[0], edges[-1]] (and for NaN)."""
    x = np.asarray(x, np.float64)
    b = np.searchsorted(edges, x, "right") - 1
    b = np.where(x == edges[-1], len(edges) - 2, b)
    with np.errstate(invalid="ignore"):
        return np.where((x >= edges[0]) & (x <= edges[-1]), b, -1)


def histograms(angles, pairs=(), bins1=BINS_1D, bins2=BINS_2D):
    """(hist1 [NF, bins1], hist2 [P, bins2, bins2], dropped [NF + P]) int64: mdgen_traj_histograms."""
    angles = np.asarray(angles, np.float64)
    NF = angles.shape[1]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    e1, e2 = hist_edges(bins1), hist_edges(bins2)
    h1 = np.zeros((NF, bins1), np.int64)
    h2 = np.zeros((len(pairs), bins2, bins2), np.int64)
    dr = np.zeros(NF + len(pairs), np.int64)
    for f in range(NF):
        b = bins_of(angles[:, f], e1)
        h1[f] = np.bincount(b[b >= 0], minlength=bins1)
        dr[f] = (b < 0).sum()
    for j, (fx, fy) in enumerate(pairs):
        bx, by = bins_of(angles[:, fx], e2), bins_of(angles[:, fy], e2)
        ok = (bx >= 0) & (by >= 0)
        h2[j] = np.bincount(bx[ok] * bins2 + by[ok], minlength=bins2 * bins2).reshape(bins2, bins2)
        dr[NF + j] = (~ok).sum()
    return h1, h2, dr


def numpy_histograms(angles, pairs=(), bins1=BINS_1D, bins2=BINS_2D):
    """The same three arrays from the installed NumPy's np.histogram / np.histogram2d on the values widened to fp64 (which is
    what the kernel bins; NumPy's own handling of an fp32 array against Python-float edges differs between its versions)."""
    angles = np.asarray(angles, np.float64)
    NF = angles.shape[1]
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    rng = (-np.pi, np.pi)
    h1 = np.stack([np.histogram(angles[:, f], range=rng, bins=bins1)[0] for f in range(NF)]).astype(np.int64) \
        if NF else np.zeros((0, bins1), np.int64)
    h2 = np.zeros((len(pairs), bins2, bins2), np.int64)
    for j, (fx, fy) in enumerate(pairs):
        h2[j] = np.histogram2d(angles[:, fx], angles[:, fy], range=(rng, rng), bins=bins2)[0]
    dr = np.concatenate([angles.shape[0] - h1.sum(1), angles.shape[0] - h2.sum((1, 2))]).astype(np.int64)
    return h1, h2, dr


def acov_fft(angles, K):
    """fp64 (acov [NF, K + 1], mean_sin, mean_cos) through a zero-padded FFT of sin and cos of the (fp32) angles."""
    a = np.asarray(angles, np.float64)
    n = a.shape[0]
    m = 1 << int(np.ceil(np.log2(2 * n)))
    out = np.zeros((a.shape[1], K + 1))
    for x in (np.sin(a), np.cos(a)):
        f = np.fft.rfft(x, m, axis=0)
        out += np.fft.irfft(f * np.conj(f), m, axis=0)[:K + 1].T
    return out / (n - np.arange(K + 1)), np.sin(a).mean(0), np.cos(a).mean(0)


def acov_direct(angles, K):
    """The definition, by a double loop."""
    a = np.asarray(angles, np.float64)
    n, NF = a.shape
    out = np.zeros((NF, K + 1))
    for f in range(NF):
        for k in range(K + 1):
            for t in range(n - k):
                out[f, k] += np.sin(a[t, f]) * np.sin(a[t + k, f]) + np.cos(a[t, f]) * np.cos(a[t + k, f])
            out[f, k] /= n - k
    return out


def acov_floor(angles, K, lags=None):
    """The largest error, over `lags` (default: all), of the sum evaluated by np.dot in fp32 on fp32 sin / cos."""
    a = np.asarray(angles, np.float64)
    n, NF = a.shape
    ref = acov_fft(angles, K)[0]
    s, c = np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)
    lags = range(K + 1) if lags is None else lags
    worst = 0.0
    for f in range(NF):
        for k in lags:
            v = (np.dot(s[:n - k, f], s[k:, f]) + np.dot(c[:n - k, f], c[k:, f])) / np.float32(n - k)
            assert v.dtype == np.float32
            worst = max(worst, abs(float(v) - ref[f, k]))
    return worst


def acov_gate(angles, K, lags=None):
    return max(32 * acov_floor(angles, K, lags), EPS32)


def decorrelation(angles, K):
    acov, ms, mc = acov_fft(angles, K)
    base = (ms * ms + mc * mc)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (acov - base) / (1.0 - base)


def analyze(traj_atom14, ref_atom14, aatype, nlag=NLAG, ref_nlag=None, pairs=DEFAULT_PAIRS, decorr=True, angles=None):
    """mdgen_amd.analysis.analyze.  `angles`: (traj, ref) angle arrays to use instead of the fp64 dihedrals -- the device's own
    fp32 angles, so that an end-to-end comparison of counts is exact."""
    labels, quad = torsion_features(aatype)
    NF = len(labels)
    a_traj, a_ref = angles if angles is not None else (dihedrals(traj_atom14, quad), dihedrals(ref_atom14, quad))
    pairs = [(a, b) for a, b in pairs if a < NF and b < NF]
    out = {"features": list(labels), "JSD": {}}
    t1, t2, _ = histograms(a_traj, pairs)
    r1, r2, _ = histograms(a_ref, pairs)
    for i, lab in enumerate(labels):
        out["JSD"][lab] = jsd(r1[i], t1[i])
    for j, (a, b) in enumerate(pairs):
        out["JSD"][labels[a] + "|" + labels[b]] = jsd(r2[j], t2[j])
    if decorr:
        k, k_ref = min(nlag, len(a_traj) - 1), min(MD_NLAG if ref_nlag is None else ref_nlag, len(a_ref) - 1)
        our, md = decorrelation(a_traj, k).astype(np.float32), decorrelation(a_ref, k_ref).astype(np.float32)
        out["our_decorrelation"] = {lab: our[i] for i, lab in enumerate(labels)}
        out["md_decorrelation"] = {lab: md[i] for i, lab in enumerate(labels)}
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------
ALL_TYPES_4 = ["ARND", "CQEG", "HILK", "MFPS", "TWYV"]       # five 4-residue sequences: every residue type once
ORDER = "ARNDCQEGHILKMFPSTWYV"


def aatype_of(seq):
    return np.array([ORDER.index(c) for c in seq], np.int64)


def mixed_types(L):
    return (np.arange(L) * 7 + 3) % 20


DIHEDRAL_F = (1, 63, 64, 65, 257, 4099)
DIHEDRAL_L = (1, 2, 4, 33)


def grid_sequence(L):
    """The sequence of the (F, L) grid of dihedral cases: ARG alone (four chi angles), TRP-LYS, FLRH, every type at L = 33."""
    return {1: aatype_of("R"), 2: aatype_of("WK"), 4: aatype_of("FLRH")}.get(L, mixed_types(L))


def peptide(F, aatype, seed=0, walk=None):
    """atom14 float32 [F, L, 14, 3]: ideal residue geometry (the oracle's frames + torsions -> atoms) on a chain of CA-like
    spacing, every coordinate perturbed by 0.05 A.  `walk` None: every frame independent; a float: frames, translations and
    torsion angles take Gaussian steps of that size (radians; 4 x in A) from frame to frame -- a trajectory."""
    import torch
    from oracle import mdgen_oracle as O
    aatype = np.asarray(aatype, np.int64)
    L = len(aatype)
    gen = torch.Generator().manual_seed(seed)
    if walk is None:
        q = torch.randn(F, L, 4, generator=gen, dtype=torch.float64)
        ang = 2 * np.pi * torch.rand(F, L, 7, generator=gen, dtype=torch.float64)
        step = torch.randn(F, L, 3, generator=gen, dtype=torch.float64)
    else:
        q = torch.randn(1, L, 4, generator=gen, dtype=torch.float64) + torch.cumsum(
            walk * torch.randn(F, L, 4, generator=gen, dtype=torch.float64), 0)
        ang = 2 * np.pi * torch.rand(1, L, 7, generator=gen, dtype=torch.float64) + torch.cumsum(
            walk * torch.randn(F, L, 7, generator=gen, dtype=torch.float64), 0)
        step = torch.randn(1, L, 3, generator=gen, dtype=torch.float64) + torch.cumsum(
            0.1 * walk * torch.randn(F, L, 3, generator=gen, dtype=torch.float64), 0)
    trans = torch.cumsum(3.8 * step / step.norm(dim=-1, keepdim=True), 1)
    rots = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
    sc = torch.stack([torch.sin(ang), torch.cos(ang)], -1)
    seqres = torch.from_numpy(aatype)[None, None].expand(1, F, L)
    a = O.frames_torsions_to_atom14(rots[None], trans[None], sc[None], seqres)[0].double()
    a = a + 0.05 * torch.randn(a.shape, generator=gen, dtype=torch.float64)
    a = a * torch.from_numpy(_atom14_mask()[aatype])[None, :, :, None]
    return a.numpy().astype(np.float32)


def _atom14_mask():
    from mdgen_amd.pdb import residue_tables
    return np.asarray(residue_tables()["atom14_mask"], np.float64)


@functools.lru_cache(maxsize=None)
def dihedral_case(F, seq_key, seed):
    """(atom14, aatype, labels, quad, fp64 angles, compared mask, gate) of a peptide case; cached, read-only."""
    aatype = np.array(seq_key, np.int64)
    labels, quad = torsion_features(aatype)
    a = peptide(F, aatype, seed)
    ref, well = dihedral_parts(a, quad)
    if well.size:
        assert (~well).mean() <= 0.01, f"{(~well).mean():.3%} of the quadruples are ill-conditioned"
        floor = float(wrapped(dihedrals_torch32(a, quad), ref)[well].max())
    else:
        floor = 0.0
    for x in (a, ref, well):
        x.setflags(write=False)
    return a, aatype, labels, quad, ref, well, max(32 * floor, EPS32)


def edge_angles():
    """float32 [n, 2]: every float32(edge) of the 100-bin and of the 50-bin table with its two float32 neighbours, +-float32(pi)
    and 0, in the first column; the same values in another order in the second."""
    v = [np.float32(0), PI32, -PI32]
    for e in np.concatenate([hist_edges(BINS_1D), hist_edges(BINS_2D)]):
        x = np.float32(e)
        v += [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    v = np.array(v, np.float32)
    return np.stack([v, np.roll(v[::-1], 7)], 1)


def random_angles(n, NF, seed, walk=0.3):
    """float32 [n, NF] in (-pi, pi]: wrapped random walks with a per-feature drift and step."""
    g = np.random.default_rng(seed)
    x = np.cumsum(g.normal(size=(n, NF)) * walk * (0.2 + g.random(NF)) + 0.01 * g.normal(size=NF), 0) + 6 * g.random(NF)
    return np.arctan2(np.sin(x), np.cos(x)).astype(np.float32)
