"""NumPy fp64 restatement of mdgen_ens_sasa_counts (csrc/k_ensemble.hip k_sasa, include/mdgen_amd.h) and of the surface entries of
mdgen_amd/ensemble.py's `analyze_ensemble(sasa=True)`, with the cases and the gates of tests/test_sasa_cpu.py and
tests/test_sasa_gpu.py.  eps32 = 2^-23.  The inputs are fp32 arrays; every reference value is computed in fp64 from those values.

Counts.  R_i = radius_i + probe and R2_j = R_j R_j are the fp32-rounded values taken to fp64 (an atom of radius 0 does not exist).
The reference computes q = c_i + R_i u_k and d2 = |q - c_j|^2 in fp64.
  device error on q  three FMAs, each within eps32 / 2 of a value of size <= max|c_i| + R_i (1 + 1e-3): the device's q is within
                     e = sqrt(3) eps32 (max|c_i| + R_i) of the reference's.  Where the coordinates themselves carry an error of up
                     to g a coordinate (the superposed coordinates of `analyze_ensemble`), q - c_j moves by up to 2 sqrt(3) g more:
                     that is added to e (as `contact_reference`'s coord_err is for contacts).
  decided test       the fp32 d2 of three differences and three fused terms is within 4 eps32 d2 of the exact one of the device's
                     q, which is within 2 sqrt(d2) e + e^2 of the reference's: a test (i, k, j) is decided when
                     |d2 - R2_j| > 8 eps32 max(d2, R2_j) + 2 sqrt(d2) e + e^2.
  point status       surely buried: a decided test buries it.  Surely exposed: every test is decided and none buries it.  Undecided
                     otherwise.
  gate               sure[f][i] <= counts_dev[f][i] <= sure[f][i] + undecided[f][i]: equality wherever undecided is 0.
  cap                the undecided share of all (frame, existing atom, point) triples is at most 1e-3: a condition on the inputs,
                     asserted on the CPU on the reference alone.
The reference tests atom i's points against the atoms with |c_i - c_j| < (R_i + R_j) 1.01 + 4 e + 1e-3 only.  Every other j is
decided and buries nothing: a point is within R_i (1 + 1e-3) of c_i, so s = sqrt(d2) >= R_j + delta with delta >= 0.009 (R_i + R_j)
+ 4 e + 1e-3, and d2 - R2_j >= delta s exceeds the margin 8 eps32 s^2 + 2 s e + e^2 (for delta < s: 8 eps32 s < 1e-3 up to
s = 1000 A, and beyond, delta = s - R_j >= s - 19 itself exceeds it).  `reference(..., cull=False)` tests every atom, and the CPU
test compares the two.

Generator.  `case(F, A, P, probe, offset, seed)`: draws in the order x, rad, dead from default_rng([777, F, A, seed]);
side = (A / 0.05)^(1/3), x = random((F, A, 3)) side + offset rounded to fp32, rad = choice([1.7, 1.55, 1.52, 1.8], A); for A > 4,
dead = random(A) < 0.2, dead atoms given radius 0 and coordinates 0.

analyze_ensemble(sasa=True).  `analyze_sasa` restates the surface entries from the fp64 Kabsch superposition of ensemble_ref, with
g = the largest coordinate gate of the two superpositions as the coordinate error.  An exposure bit (frame, residue) is decided
when the area from `sure` and the area from `sure + undecided` fall on the same side of the threshold by more than 1e-9 relative;
with every bit decided the exposure bits, probabilities, the two sets, the Jaccard index and n11 are exact, the mutual information
(restated as a loop over the four cells) and Spearman's rho (scipy.stats.spearmanr) match to 1e-12, and the mean areas lie between
the means from `sure` and from `sure + undecided` (+ 1e-9 relative for the fp64 sums)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_ref as R  # noqa: E402

EPS32 = 2.0 ** -23
UNDECIDED_CAP = 1e-3
BONDI = (1.7, 1.55, 1.52, 1.8)
NEIGHBOURS = 512                # csrc/kernels.h kEnsSasaMaxNeighbours
SCAN = 64                       # the atoms a wave scans at a time
MAX_POINTS = 4096

# (F, A, P, probe, offset)
CASES = [(1, 1, 1, 1.4, 0.0), (2, 2, 7, 1.4, 0.0), (3, 63, 63, 1.4, 0.0), (2, 64, 64, 2.8, 0.0), (2, 65, 65, 1.4, 0.0),
         (2, 257, 96, 2.8, 0.0), (1, 3584, 15, 2.8, 0.0), (1, 1025, 33, 1.4, 100.0), (5, 56, 960, 1.4, 0.0)]
# the number of points at the wave's edge and at the limit, at small A
POINT_CASES = [(2, 20, 63, 1.4, 0.0), (2, 20, 64, 1.4, 0.0), (2, 20, 65, 1.4, 0.0), (1, 20, 4096, 1.4, 0.0)]
# (A, P): every atom within reach of every other (`dense_case`), so that an atom has A - 1 neighbours: the list holds 512
DENSE_CASES = [(NEIGHBOURS - 1, 33), (NEIGHBOURS, 33), (NEIGHBOURS + 1, 33), (NEIGHBOURS + 2, 33)]
DENSE_SIDE = 4.9                # the box's diagonal, 8.49 A, is below the smallest reach 2 (1.52 + 2.8) = 8.64 A
DENSE_PROBE = 2.8
ANALYZE = dict(L=12, T=33, F=65, seed=0)
ANALYZE_SETTINGS = dict(n_points=96, probe=2.8, sasa_threshold=40.0)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def sphere_points(n):
    """The golden-section spiral, point by point."""
    out = np.empty((n, 3))
    for i in range(n):
        y = (2 * i + 1) / n - 1
        r = np.sqrt(1 - y * y)
        phi = i * (np.pi * (3 - np.sqrt(5.0)))
        out[i] = (np.cos(phi) * r, y, np.sin(phi) * r)
    return out.astype(np.float32)


def case(F, A, P, probe, offset, seed=0):
    """(x fp32 [F, A, 3], radius fp32 [A], points fp32 [P, 3], probe)."""
    g = np.random.default_rng([777, F, A, seed])
    side = (A / 0.05) ** (1.0 / 3.0)
    x = (g.random((F, A, 3)) * side + offset).astype(np.float32)
    rad = g.choice(np.array(BONDI), A).astype(np.float32)
    if A > 4:
        dead = g.random(A) < 0.2
        rad[dead] = 0.0
        x[:, dead] = 0.0
    return x, rad, sphere_points(P), probe


def dense_case(A, P, seed=0):
    """One frame of A existing atoms in a box of DENSE_SIDE: each is within reach of every other."""
    g = np.random.default_rng([778, A, seed])
    x = (g.random((1, A, 3)) * DENSE_SIDE).astype(np.float32)
    rad = g.choice(np.array(BONDI), A).astype(np.float32)
    return x, rad, sphere_points(P), DENSE_PROBE


def clump_case(ball=1.0, seed=0):
    """About 300 existing atoms within a ball of radius `ball` (340 slots, a tenth of them dead) and 20 scattered around it."""
    g = np.random.default_rng([779, seed])
    n = 340
    v = g.normal(size=(n, 3))
    v *= (ball * g.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    far = g.random((20, 3)) * 30.0 - 15.0
    x = (np.concatenate([v, far], 0) + 20.0)[None].astype(np.float32)
    rad = g.choice(np.array(BONDI), n + 20).astype(np.float32)
    dead = np.flatnonzero(g.random(n) < 0.1)
    rad[dead] = 0.0
    x[:, dead] = 0.0
    return x, rad, sphere_points(33), 1.4


def big_clump_case(seed=0):
    """700 existing atoms within a 1.5 A ball and 20 scattered: every clump atom has more neighbours than the list holds."""
    g = np.random.default_rng([780, seed])
    n = 700
    v = g.normal(size=(n, 3))
    v *= (1.5 * g.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    far = g.random((20, 3)) * 30.0 - 15.0
    x = (np.concatenate([v, far], 0) + 20.0)[None].astype(np.float32)
    rad = g.choice(np.array(BONDI), n + 20).astype(np.float32)
    return x, rad, sphere_points(33), 1.4


# ---- the counts ------------------------------------------------------------------------------------------------------
def radii(radius, probe):
    """(R, R2) fp64 [A] of the fp32 values: R = radius + probe, R2 = R R, each rounded to fp32; 0 where radius is 0."""
    radius = np.asarray(radius, np.float32)
    R = np.where(radius != 0, radius + np.float32(probe), np.float32(0)).astype(np.float32)
    return R.astype(np.float64), (R * R).astype(np.float32).astype(np.float64)


def reference(x, radius, points, probe, coord_err=0.0, cull=True):
    """(sure, undecided) int64 [F, A]: the points of every atom that are surely exposed, and those that are undecided.  x: the
    device's fp32 input, or fp64 coordinates within `coord_err` a coordinate of it."""
    x = np.asarray(x, np.float64)
    u = np.asarray(points, np.float32).astype(np.float64)
    Rv, R2 = radii(radius, probe)
    F, A = x.shape[:2]
    live = np.flatnonzero(Rv > 0)
    sure, und = np.zeros((F, A), np.int64), np.zeros((F, A), np.int64)
    for f in range(F):
        c = x[f, live]
        for n, i in enumerate(live):
            e = np.sqrt(3.0) * EPS32 * (np.abs(c[n]).max() + Rv[i]) + 2.0 * np.sqrt(3.0) * coord_err
            other = np.ones(len(live), bool)
            other[n] = False
            if cull:
                dist = np.sqrt(((c - c[n]) ** 2).sum(-1))
                other &= dist < (Rv[i] + Rv[live]) * 1.01 + 4 * e + 1e-3
            q = c[n] + Rv[i] * u                                                # [P, 3]
            d2 = ((q[:, None, :] - c[other][None, :, :]) ** 2).sum(-1)          # [P, n]
            r2 = R2[live][other][None, :]
            decided = np.abs(d2 - r2) > 8 * EPS32 * np.maximum(d2, r2) + 2.0 * np.sqrt(d2) * e + e * e
            buried = (decided & (d2 < r2)).any(1)
            exposed = decided.all(1) & ~(d2 < r2).any(1)
            sure[f, i] = exposed.sum()
            und[f, i] = (~buried & ~exposed).sum()
    return sure, und


def undecided_share(und, radius, P):
    return und.sum() / max(1, und.shape[0] * int((np.asarray(radius) != 0).sum()) * P)


def brute_counts(x, radius, points, probe):
    """The definition as it stands, in fp32 with NumPy's own rounding (no fused multiply-add): what a plain restatement gives.  Not
    a gate -- borderline points may differ from the device -- but equal to it wherever nothing is undecided."""
    x = np.asarray(x, np.float32)
    u = np.asarray(points, np.float32)
    Rv, R2 = radii(radius, probe)
    Rv, R2 = Rv.astype(np.float32), R2.astype(np.float32)
    F, A = x.shape[:2]
    out = np.zeros((F, A), np.int64)
    for f in range(F):
        for i in np.flatnonzero(Rv > 0):
            q = x[f, i] + Rv[i] * u
            d2 = ((q[:, None, :] - x[f][None, :, :]) ** 2).sum(-1)
            hit = d2 < R2[None, :]
            hit[:, i] = False
            out[f, i] = (~hit.any(1)).sum()
    return out


# ---- the host estimators, restated -----------------------------------------------------------------------------------
def atom_radii(aatype):
    from mdgen_amd.pdb import residue_tables
    t = residue_tables()
    element = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}
    out = np.zeros((len(aatype), 14), np.float32)
    for r, aa in enumerate(np.asarray(aatype)):
        for s in range(14):
            if t["atom14_mask"][aa, s] != 0:
                out[r, s] = element[str(t["atom_types"][t["atom14_to_atom37"][aa, s]])[0]]
    return out.reshape(-1)


def mi_loop(bits):
    """Mutual information (nats) of every pair of columns of bits [F, L], cell by cell."""
    bits = np.asarray(bits, bool)
    F, L = bits.shape
    out = np.zeros((L, L))
    for i in range(L):
        for j in range(L):
            for a in (False, True):
                for b in (False, True):
                    pab = np.mean((bits[:, i] == a) & (bits[:, j] == b))
                    if pab > 0:
                        out[i, j] += pab * np.log(pab / (np.mean(bits[:, i] == a) * np.mean(bits[:, j] == b)))
    return out


def residue_matrix(aatype, probe, n_points, atoms="sidechain"):
    """M fp64 [14 L, L]: M[a][res(a)] = 4 pi R_a^2 / n of the selected existing atoms."""
    L = len(aatype)
    Rv, _ = radii(atom_radii(aatype), probe)
    m = np.zeros((14 * L, L))
    for a in range(14 * L):
        if Rv[a] > 0 and (atoms == "all" or a % 14 >= 4):
            m[a, a // 14] = 4.0 * np.pi * Rv[a] * Rv[a] / n_points
    return m


def analyze_sasa(traj, ref, aatype, probe=2.8, n_points=960, sasa_threshold=2.0, sasa_atoms="sidechain", fit="heavy"):
    """(out, aux): the surface entries of mdgen_amd.ensemble.analyze_ensemble(sasa=True) in fp64, and what the gates need: aux["lo"] /
    aux["hi"] the residue areas [frames, L] from `sure` / `sure + undecided` of (sampled, MD), aux["decided"] whether every exposure
    bit is decided, aux["undecided"] the undecided points of each ensemble, aux["n11"] the joint counts."""
    traj, ref = np.asarray(traj, np.float32), np.asarray(ref, np.float32)
    L = len(aatype)
    w, ex = R.fit_weights(aatype, fit)
    x, r = traj.reshape(len(traj), -1, 3), ref.reshape(len(ref), -1, 3)
    kx, kr = R.kabsch(x, r[0], w), R.kabsch(r, r[0], w)
    g = max(R.coordinate_gate(x, kx).max(), R.coordinate_gate(r, kr).max())
    xs, rs = R.superposed(x, kx, ex), R.superposed(r, kr, ex)
    rad, pts, m = atom_radii(aatype), sphere_points(n_points), residue_matrix(aatype, probe, n_points, sasa_atoms)
    out, aux = {}, {"g": g, "lo": [], "hi": [], "undecided": [], "n11": [], "decided": True}
    bits = {}
    for pre, c in (("", xs), ("ref_", rs)):
        # (the superposed coordinates are fp64 here and fp32 on the device, within g of each other: the gate's coord_err)
        sure, und = reference(c, rad, pts, probe, g)
        lo, hi = sure @ m, (sure + und) @ m
        aux["lo"].append(lo), aux["hi"].append(hi), aux["undecided"].append(int(und.sum()))
        side_lo, side_hi = lo - sasa_threshold, hi - sasa_threshold
        ok = (np.sign(side_lo) == np.sign(side_hi)) & (np.minimum(np.abs(side_lo), np.abs(side_hi)) > 1e-9 * abs(sasa_threshold))
        aux["decided"] = aux["decided"] and bool(ok.all())
        bits[pre] = lo > sasa_threshold
        out[pre + "exposure_prob"] = bits[pre].sum(0) / float(len(c))
        out[pre + "residue_sasa_mean"] = 0.5 * (lo.mean(0) + hi.mean(0))
        aux["n11"].append(bits[pre].astype(np.int64).T @ bits[pre].astype(np.int64))
    aux["bits"] = (bits[""], bits["ref_"])
    in_ref = bits["ref_"][0]
    sets = [~in_ref & (out[k] > 0.1) for k in ("ref_exposure_prob", "exposure_prob")]
    aux["sets"] = sets
    out["exposed_residue_jaccard"] = R.jaccard_loop(sets[0], sets[1])
    out["exposed_mi"], out["ref_exposed_mi"] = mi_loop(bits[""]), mi_loop(bits["ref_"])
    iu = np.triu_indices(L, 1)
    import warnings
    from scipy.stats import spearmanr
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # (a constant side: NaN, as `spearman` gives)
        out["exposed_mi_spearman"] = float(spearmanr(out["exposed_mi"][iu], out["ref_exposed_mi"][iu])[0])
    return out, aux
