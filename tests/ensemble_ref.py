"""NumPy fp64 restatement of csrc/k_ensemble.hip (mdgen_ens_superpose / _moments / _pairwise_d2 / _contact_counts, include/mdgen_amd.h)
and of mdgen_amd/ensemble.py's `analyze_ensemble`, with the cases and the gates of tests/test_ensemble_cpu.py and
tests/test_ensemble_gpu.py.  eps32 = 2^-23, eps64 = 2^-52.  The inputs are fp32 arrays; every reference value is computed in fp64
from those fp32 values.

Superposition.  Reference: Kabsch -- numpy.linalg.svd of H = sum w (x - cx)(ref - cr)^T = U S V^T, R = V diag(1, 1, d) U^T with
d = sign det H, taken as det U det V (the same sign, and defined where three weighted atoms make H singular).  (With H_ij = sum w a_i b_j the rotation taking a to b is V D U^T.)
  rotation gate      the first-order perturbation of the optimal rotation under a perturbation E of H is bounded by
                     |E| / (s2 + d s3); the device forms H in fp64 (|E| ~ eps64 s1), so max |R_dev - R_ref| <= 1e3 eps64 s1 /
                     (s2 + d s3), three orders over the bound.  A case is well posed when (s2 + d s3) / s1 >= 1e-3: asserted for
                     every frame on the CPU; the gate is then at most 2.3e-10.  det R and R R^T within 1e-12 of 1 and I.
  coordinate gate    out = fma chain of fp32(R) and the fp32 difference x - fp32(cx), ending on fp32(cr): the centroid's rounding
                     (eps32 / 2 |cx|), the subtraction (eps32 / 2 |d|), R's rounding (eps32 / 2 per entry, |R| <= 1) and three
                     FMAs (eps32 / 2 each on a partial sum <= |d|_1 + |cr_i|) together err by at most eps32 (2.5 |x_a - cx|_1 +
                     0.5 |cx|_1 + 1.5 |cr_i|).  Gate: 4 eps32 (|x_a - cx|_1 + |cx|_1 + |cr|_1) + rotation gate x |x_a - cx|_1.
  rmsd gate          relative 1e-9 against fp64 (the objective is stationary at R: the rotation gate enters squared); where the
                     true value is 0 -- the identity frame -- absolute 1e-6 x the coordinate scale (10).

Moments.  Reference: the two-pass fp64 mean and covariance (divided by F).  The device adds u = x - x_0 and u_i u_j in fp64, F terms
in a few partial sums: with g = max(1e-12, 4 F eps64), cov within g (mean|u_i u_j| + mean|u_i| mean|u_j|), mean within
g mean|u_i| + 2 eps64 |mean_i| (the last addition x_0 + mean(u)).

Pairwise d2.  The fp32 difference is exact to eps32 / 2 relative, so its square to eps32 (1 + eps32 / 4); 3A non-negative terms
added by FMAs lose at most 3A eps32 / 2 relative more: every pair within (3A + 2) eps32 d2_64.  A self-comparison's diagonal is
exactly 0.  sums against fp64 sums of the device's own matrix: max(1e-12, 4 Fa Fb eps64) relative.

Contacts.  The fp32 d2 of three differences and three fused terms is within 4 eps32 d2 of fp64: a (t, i, j) is decided when
|d2_64 - c2| > 8 eps32 max(d2_64, c2) (+ the effect of a coordinate error, when the coordinates themselves carry one), and then its
contribution must match: |counts_dev - counts_decided_ref| <= undecided[i][j].  The undecided share is capped at 1e-3.

analyze_ensemble.  With g the largest coordinate gate of the two superpositions: an RMSF, a pair's RMSD and a Gaussian W2 (a metric
on distributions) move by at most 2 sqrt(3) g when every coordinate moves by at most g; the other gates are in `analyze_gates`."""
import numpy as np

EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
SCALE = 10.0
WELL_POSED = 1e-3
UNDECIDED_CAP = 1e-3
CUTOFF = 8.0
CA = 1

# (F, A, weights, exists): weights "uniform" | "three" (0 / 1, three atoms weighted) | "ramp" (non-uniform); exists: zeros in it
SUPERPOSE_CASES = [(1, 3, "uniform", False), (2, 4, "ramp", True), (65, 56, "uniform", True), (3, 63, "three", False),
                   (3, 64, "ramp", False), (3, 65, "uniform", False), (257, 257, "ramp", True), (5, 3584, "uniform", True),
                   (4099, 56, "three", True)]
MOMENTS_CASES = [(1, 1, 0.0), (2, 3, 0.0), (65, 56, 0.0), (257, 65, 100.0), (4099, 257, 0.0), (100003, 4, 0.0)]   # (F, A, offset)
# (Fa, Fb, A); Fb None: xa against itself, one pointer.  The last three straddle the kernel's tile: 128 x 64 frames, 24 coordinates
PAIRWISE_CASES = [(1, 1, 1), (2, 3, 1), (63, 65, 3), (64, 64, 4), (65, 129, 56), (257, 250, 256), (250, 250, 1024),
                  (65, None, 56), (257, None, 256), (127, 63, 7), (128, 64, 8), (129, 65, 9)]
CONTACT_CASES = [(1, 1), (1, 2), (3, 63), (3, 65), (65, 64), (257, 257), (17, 1024)]
ANALYZE_CASE = dict(L=8, T=33, F=129)


def _rng(*key):
    return np.random.default_rng([20240607, *[int(k) for k in key]])


def random_rotation(g):
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---- superposition ---------------------------------------------------------------------------------------------------
def superpose_case(F, A, weights, with_exists):
    """(x fp32 [F, A, 3], ref fp32 [A, 3], w fp32 [A], exists uint8 [A] or None).  frame = rotation (ref + 1 A noise) + translation
    of a cloud of scale 10 A (axes 12, 10, 8); where F allows, frame 0 is ref itself, frames 1-3 are rotations by exactly pi about
    x, y, z, frame 4 is translated by 100 A and frame 5 is a mirror image of ref."""
    g = _rng(1, F, A)
    ref = (g.normal(size=(A, 3)) * np.array([12.0, 10.0, 8.0]) + g.normal(size=3) * SCALE).astype(np.float32)
    x = np.empty((F, A, 3))
    for f in range(F):
        body = ref.astype(np.float64) + g.normal(size=(A, 3))
        rot, shift = random_rotation(g), g.normal(size=3) * SCALE
        if f == 0 and F > 1:
            x[f] = ref
            continue
        if f in (1, 2, 3) and F > 3:
            rot = -np.eye(3)
            rot[f - 1, f - 1] = 1.0
        if f == 4:
            shift = np.array([100.0, -100.0, 100.0])
        if f == 5:
            body = body * np.array([-1.0, 1.0, 1.0])
        x[f] = body @ rot.T + shift
    x = x.astype(np.float32)
    if weights == "uniform":
        w = np.ones(A, np.float32)
    elif weights == "three":
        w = np.zeros(A, np.float32)
        w[g.choice(A, 3, replace=False)] = 1.0
    else:
        w = (0.25 + g.random(A) * 4.0).astype(np.float32)
    exists = None
    if with_exists:
        exists = (g.random(A) < 0.7).astype(np.uint8)
        keep = np.flatnonzero(w)[:3]
        exists[keep] = 1
        if exists.all():
            exists[np.setdiff1d(np.arange(A), keep)[0]] = 0
        x[:, exists == 0] = 0.0                     # padding slots hold zeros ...
        ref = ref.copy()
        ref[exists == 0] = 0.0
        w = (w * exists).astype(np.float32)         # ... and carry no weight
        if weights == "three":
            assert (w > 0).sum() == 3
    return x, ref, w, exists


def kabsch(x, ref, w):
    """fp64 Kabsch of frames x [F, A, 3] on ref [A, 3] under w [A]: dict of R [F, 3, 3], cx [F, 3], cr [3], s [F, 3] (singular values
    of H, descending), d [F] (sign det H), rmsd [F]."""
    x, ref, w = np.asarray(x, np.float64), np.asarray(ref, np.float64), np.asarray(w, np.float64)
    W = w.sum()
    cx = (x * w[None, :, None]).sum(1) / W
    cr = (ref * w[:, None]).sum(0) / W
    p, q = x - cx[:, None, :], ref - cr
    H = np.einsum("a,fai,aj->fij", w, p, q)
    U, s, Vt = np.linalg.svd(H)
    d = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)   # sign det H, and definite where H is singular
    D = np.stack([np.ones_like(d), np.ones_like(d), d], -1)
    R = np.einsum("fji,fj,fkj->fik", Vt, D, U)          # V D U^T
    res = np.einsum("fij,faj->fai", R, p) - q
    rmsd = np.sqrt((w[None, :] * (res ** 2).sum(-1)).sum(1) / W)
    return {"R": R, "cx": cx, "cr": cr, "s": s, "d": d, "rmsd": rmsd}


def objective(R, x, ref, w, cx, cr):
    """sum w |R (x - cx) - (ref - cr)|^2 of one frame."""
    res = (np.asarray(x, np.float64) - cx) @ np.asarray(R).T - (np.asarray(ref, np.float64) - cr)
    return float((np.asarray(w, np.float64) * (res ** 2).sum(-1)).sum())


def well_posedness(k):
    return (k["s"][:, 1] + k["d"] * k["s"][:, 2]) / k["s"][:, 0]


def rotation_gate(k):
    return 1e3 * EPS64 / well_posedness(k)              # [F]


def superposed(x, k, exists=None):
    """The fp64 superposed coordinates R (x - cx) + cr; atoms with exists == 0 unchanged."""
    x = np.asarray(x, np.float64)
    out = np.einsum("fij,faj->fai", k["R"], x - k["cx"][:, None, :]) + k["cr"]
    if exists is not None:
        out[:, np.asarray(exists) == 0] = x[:, np.asarray(exists) == 0]
    return out


def coordinate_gate(x, k):
    """[F, A]: 4 eps32 (|x_a - cx|_1 + |cx|_1 + |cr|_1) + rotation gate x |x_a - cx|_1."""
    d1 = np.abs(np.asarray(x, np.float64) - k["cx"][:, None, :]).sum(-1)
    return 4 * EPS32 * (d1 + np.abs(k["cx"]).sum(-1)[:, None] + np.abs(k["cr"]).sum()) + rotation_gate(k)[:, None] * d1


# ---- moments ---------------------------------------------------------------------------------------------------------
def moments_case(F, A, offset):
    g = _rng(2, F, A)
    base = g.normal(size=(A, 3)) * SCALE + offset
    mix = g.normal(size=(A, 3, 3)) * 0.7
    x = base[None] + np.einsum("aij,faj->fai", mix, g.normal(size=(F, A, 3)))
    return x.astype(np.float32)


def moments(x):
    """Two-pass fp64: (mean [A, 3], cov [A, 3, 3]) over the frames, divided by F."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    y = x - mean
    return mean, np.einsum("fai,faj->aij", y, y) / x.shape[0]


def moments_gates(x):
    """(mean gate [A, 3], cov gate [A, 3, 3])."""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    u = x - x[0]
    g = max(1e-12, 4 * F * EPS64)
    au = np.abs(u).mean(0)
    cov_gate = g * (np.abs(np.einsum("fai,faj->faij", u, u)).mean(0) + au[:, :, None] * au[:, None, :])
    return g * au + 2 * EPS64 * np.abs(x.mean(0)), cov_gate


# ---- pairwise --------------------------------------------------------------------------------------------------------
def pairwise_case(Fa, Fb, A):
    g = _rng(3, Fa, Fb or 0, A)
    base = g.normal(size=(A, 3)) * SCALE
    xa = (base + g.normal(size=(Fa, A, 3)) * 1.5).astype(np.float32)
    xb = None if Fb is None else (base + g.normal(size=(Fb, A, 3)) * 1.5).astype(np.float32)
    return xa, xb


def pairwise_d2(xa, xb):
    """fp64 [Fa, Fb]: sum over atoms and axes of (xa_i - xb_j)^2, the direct form (row by row: no Fa x Fb x 3A array)."""
    a = np.asarray(xa, np.float64).reshape(len(xa), -1)
    b = np.asarray(xb, np.float64).reshape(len(xb), -1)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        out[i] = ((a[i] - b) ** 2).sum(1)
    return out


def pairwise_sums(d2, A):
    d2 = np.asarray(d2, np.float64)
    return np.array([np.sqrt(d2 / A).sum(), (d2 / A).sum()])


# ---- contacts --------------------------------------------------------------------------------------------------------
def contact_box(N):
    """Side of the box in which N uniform points have about 20 % of their pairs within 8 A (edge effects included)."""
    return 18.5


def contact_case(F, N):
    g = _rng(4, F, N)
    return (g.random(size=(F, N, 3)) * contact_box(N)).astype(np.float32)


def cutoff2(cutoff=CUTOFF):
    return np.float64(np.float32(np.float64(cutoff) * np.float64(cutoff)))


def contact_reference(ca, cutoff=CUTOFF, coord_err=0.0):
    """(counts of the decided (t, i, j) that are contacts, undecided counts) int64 [N, N], frame by frame.  `coord_err`: a bound on
    the error every coordinate of `ca` carries (0: the coordinates are the device's inputs)."""
    ca = np.asarray(ca, np.float64)
    c2 = cutoff2(cutoff)
    N = ca.shape[1]
    yes, und = np.zeros((N, N), np.int64), np.zeros((N, N), np.int64)
    e = 2.0 * np.sqrt(3.0) * coord_err                     # a pair's distance moves by at most this
    for t in range(ca.shape[0]):
        diff = ca[t][:, None, :] - ca[t][None, :, :]
        d2 = (diff ** 2).sum(-1)
        margin = 8 * EPS32 * np.maximum(d2, c2) + (2.0 * np.sqrt(d2) * e + e * e if coord_err else 0.0)
        decided = np.abs(d2 - c2) > margin
        if coord_err == 0.0:
            decided |= np.eye(N, dtype=bool)               # a residue with itself: exactly 0 on the device too
        yes += decided & (d2 < c2)
        und += ~decided
    return yes, und


# ---- host estimators, restated by other formulas ---------------------------------------------------------------------
def gaussian_w2(mean_a, cov_a, mean_b, cov_b):
    """Per atom |mu_a - mu_b|^2 and tr(S_a + S_b) - 2 tr((S_a S_b)^1/2), the trace of the root as the sum of the square roots of the
    eigenvalues of the (non-symmetric) product S_a S_b."""
    trans = ((np.asarray(mean_a) - np.asarray(mean_b)) ** 2).sum(-1)
    lam = np.linalg.eigvals(np.asarray(cov_a) @ np.asarray(cov_b)).real
    cross = np.sqrt(np.maximum(lam, 0.0)).sum(-1)
    var = np.maximum(np.trace(cov_a, axis1=-2, axis2=-1) + np.trace(cov_b, axis1=-2, axis2=-1) - 2 * cross, 0.0)
    return trans, var, float(np.sqrt(np.mean(trans + var)))


def pca_fit(ca):
    """By numpy.linalg.svd of the centred data: components (rows), eigenvalues s^2 / F, sign: largest-magnitude entry positive."""
    y = np.asarray(ca, np.float64).reshape(len(ca), -1)
    mean = y.mean(0)
    _, s, vt = np.linalg.svd(y - mean, full_matrices=True)
    lam = np.zeros(y.shape[1])
    lam[:len(s)] = s ** 2 / len(y)
    vt = vt * np.sign(vt[np.arange(len(vt)), np.abs(vt).argmax(1)])[:, None]
    return {"mean": mean, "components": vt, "eigenvalues": lam, "explained": lam / lam.sum()}


def pca_project(ca, fit, k=2):
    return (np.asarray(ca, np.float64).reshape(len(ca), -1) - fit["mean"]) @ fit["components"][:k].T


def pca_w2(a, b):
    from scipy.optimize import linear_sum_assignment
    b = b[np.round(np.linspace(0, len(b) - 1, len(a))).astype(np.int64)]
    cost = ((a[:, None] - b[None]) ** 2).sum(-1)
    r, c = linear_sum_assignment(cost)
    return float(np.sqrt(cost[r, c].mean()))


def jaccard_loop(a, b):
    inter = union = 0
    for u, v in zip(np.asarray(a).ravel().tolist(), np.asarray(b).ravel().tolist()):
        inter += bool(u and v)
        union += bool(u or v)
    return inter / union if union else float("nan")


# ---- analyze_ensemble ------------------------------------------------------------------------------------------------
def analyze_case(L=8, T=33, F=129, seed=0):
    """(traj fp32 [T, L, 14, 3], ref fp32 [F, L, 14, 3], aatype [L]): a helix-like C-alpha trace with side atoms around it, an MD
    ensemble fluctuating by ~1 A with per-residue amplitudes, and a sampled ensemble with other amplitudes, each frame rotated and
    translated at random.  Padding slots (atom14_mask == 0) are zero."""
    from mdgen_amd.pdb import residue_tables
    g = _rng(5, L, T, F, seed)
    aatype = g.integers(0, 20, size=L)
    mask = np.asarray(residue_tables()["atom14_mask"])[aatype] != 0
    i = np.arange(L)
    ca = np.stack([2.3 * np.cos(i * 1.75), 2.3 * np.sin(i * 1.75), 1.5 * i], -1) * 1.6
    base = ca[:, None, :] + g.normal(size=(L, 14, 3)) * 1.8
    base[:, CA] = ca
    amp_md = 0.4 + g.random(L) * 1.2
    amp_tr = amp_md * (0.6 + g.random(L) * 0.8)

    def ensemble(n, amp):
        out = np.empty((n, L, 14, 3))
        for f in range(n):
            body = base + g.normal(size=(L, 1, 3)) * amp[:, None, None] + g.normal(size=(L, 14, 3)) * 0.3
            out[f] = body @ random_rotation(g).T + g.normal(size=3) * SCALE
        out[:, ~mask] = 0.0
        return out.astype(np.float32)
    return ensemble(T, amp_tr), ensemble(F, amp_md), aatype


def fit_weights(aatype, fit):
    from mdgen_amd.pdb import residue_tables
    mask = np.asarray(residue_tables()["atom14_mask"])[np.asarray(aatype)] != 0
    w = mask.astype(np.float64)
    if fit == "ca":
        w = np.zeros_like(w)
        w[:, CA] = 1.0
    return w.reshape(-1), mask.reshape(-1).astype(np.uint8)


def pearson(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def analyze_ensemble(traj, ref, aatype, fit="heavy", cutoff=CUTOFF, pca=True, with_aux=False, extra_err=0.0):
    """mdgen_amd.ensemble.analyze_ensemble in fp64.  `with_aux`: also what the gates need (superposed coordinates, coordinate gate,
    contact counts of the decided frames and the undecided counts).  `extra_err`: a bound on the distance between every atom of
    `traj` and the atom the device analysed, up to one rigid motion per frame (0: the device analysed `traj` itself); it is added
    to the coordinate gate."""
    traj, ref = np.asarray(traj, np.float32), np.asarray(ref, np.float32)
    L = len(aatype)
    w, ex = fit_weights(aatype, fit)
    x, r = traj.reshape(len(traj), -1, 3), ref.reshape(len(ref), -1, 3)
    target = r[0]
    kx, kr = kabsch(x, target, w), kabsch(r, target, w)
    g = max(coordinate_gate(x, kx).max(), coordinate_gate(r, kr).max()) + extra_err
    xs, rs = superposed(x, kx, ex), superposed(r, kr, ex)
    out = {}
    (mx, cx), (mr, cr) = moments(xs), moments(rs)
    exists = ex.reshape(L, 14) != 0
    for key, c in (("atom_rmsf", cx), ("ref_atom_rmsf", cr)):
        out[key] = np.where(exists, np.sqrt(np.trace(c, axis1=1, axis2=2)).reshape(L, 14), 0.0)
    out["ca_rmsf"], out["ref_ca_rmsf"] = out["atom_rmsf"][:, CA].copy(), out["ref_atom_rmsf"][:, CA].copy()
    out["rmsf_pearson"] = pearson(out["ca_rmsf"], out["ref_ca_rmsf"])
    ca_x, ca_r = xs.reshape(-1, L, 14, 3)[:, :, CA], rs.reshape(-1, L, 14, 3)[:, :, CA]
    for pre, a, b in (("", ca_x, ca_x), ("ref_", ca_r, ca_r), ("cross_", ca_x, ca_r)):
        rm = np.sqrt(pairwise_d2(a, b) / L)
        out[pre + "mean_pairwise_rmsd"], out[pre + "rms_pairwise_rmsd"] = float(rm.mean()), float(np.sqrt((rm ** 2).mean()))
    sel = np.arange(L) * 14 + CA
    trans, var, total = gaussian_w2(mx[sel], cx[sel], mr[sel], cr[sel])
    out["emd_mean"], out["emd_var"], out["emd_total"] = float(np.sqrt(trans.mean())), float(np.sqrt(var.mean())), total
    yes_x, und_x = contact_reference(ca_x, cutoff, g)
    yes_r, und_r = contact_reference(ca_r, cutoff, g)
    yes_0, und_0 = contact_reference(ca_r[:1], cutoff, g)
    out["contact_prob"], out["ref_contact_prob"] = yes_x / len(ca_x), yes_r / len(ca_r)
    if pca:
        fr = pca_fit(ca_r)
        out["pca_w2_ref"] = pca_w2(pca_project(ca_x, fr), pca_project(ca_r, fr))
        fj = pca_fit(np.concatenate([ca_r, ca_x], 0))
        out["pca_w2_joint"] = pca_w2(pca_project(ca_x, fj), pca_project(ca_r, fj))
        out["pca_explained"] = fr["explained"][:2].copy()
    aux = {"g": g, "yes": (yes_x, yes_r, yes_0), "und": (und_x, und_r, und_0), "ca": (ca_x, ca_r), "L": L}
    # the contact sets where every frame is decided; the undecided ones widen the interval in `jaccard_interval`
    up = np.triu(np.ones((L, L), bool), 1)
    sets = {}
    for name, yes, und, n in (("x", yes_x, und_x, len(ca_x)), ("r", yes_r, und_r, len(ca_r))):
        lo, hi = yes / n, (yes + und) / n
        in_lo, in_hi = yes_0 > 0, (yes_0 + und_0) > 0
        sets[name] = {"weak": (up & in_lo & (hi < 0.9), up & in_hi & (lo < 0.9)),             # (surely in, possibly in)
                      "transient": (up & ~in_hi & (lo > 0.1), up & ~in_lo & (hi > 0.1))}
    aux["sets"] = sets
    for key in ("weak", "transient"):
        lo, hi = jaccard_interval(sets["r"][key], sets["x"][key])
        out[key + "_contacts_jaccard"] = lo if lo == hi or not (lo == lo) else 0.5 * (lo + hi)
        aux[key + "_interval"] = (lo, hi)
    return (out, aux) if with_aux else out


def jaccard_interval(a, b):
    """[lowest, highest] Jaccard index of two sets given as (surely in, possibly in) boolean arrays; (nan, nan) when the union is
    surely empty."""
    (a_in, a_may), (b_in, b_may) = a, b
    i_lo, i_hi = int((a_in & b_in).sum()), int((a_may & b_may).sum())
    u_lo, u_hi = int((a_in | b_in).sum()), int((a_may | b_may).sum())
    if u_hi == 0:
        return float("nan"), float("nan")
    return i_lo / u_hi, (i_hi / u_lo if u_lo else 1.0)


def analyze_gates(ref_out, aux):
    """{key: absolute gate} of `analyze_ensemble`'s scalar and array keys but the contact ones, from g = aux["g"], the largest
    coordinate gate of the two superpositions (every superposed coordinate of the device is within g of the fp64 one):
      RMSFs              the standard deviation of a perturbed series moves by at most the perturbation's: sqrt(3) g; x 2.
      rmsf_pearson       the correlation is the dot product of two centred unit vectors; each moves by at most 2 |delta| / |a - mean|
                         with |delta| <= sqrt(L) x the RMSF gate.
      pairwise RMSDs     a pair's sqrt(d2 / A) moves by at most 2 sqrt(3) g, and the fp32 sum is within (3 A + 2) eps32 / 2 relative.
      emd_*              the Gaussian W2 is a metric, its translation and covariance (Bures) parts too: each ensemble's move costs at
                         most sqrt(3) g; 1e-7 for the host's square roots near zero.
      pca_*              e = 2 sqrt(3 N) g bounds a centred frame vector's move; the covariance moves by dC <= 2 sqrt(l1) e + e^2 in
                         norm, a component by at most 2 dC / gap (Davis-Kahan, gap: the smallest among l1 - l2, l2 - l3), a projected
                         point by e + |y|_max 2 dC / gap per axis; the optimal-assignment cost is a W2 between point sets: it moves by
                         at most the sum of the two sets' moves, sqrt(2) per 2-D point.  explained: (dC + l dS / S) / S."""
    g, L = aux["g"], aux["L"]
    rm = 2 * np.sqrt(3.0) * g
    gates = {k: rm for k in ("ca_rmsf", "ref_ca_rmsf", "atom_rmsf", "ref_atom_rmsf")}
    a, b = ref_out["ca_rmsf"], ref_out["ref_ca_rmsf"]
    gates["rmsf_pearson"] = 2 * np.sqrt(L) * rm * (1 / np.linalg.norm(a - a.mean()) + 1 / np.linalg.norm(b - b.mean())) + 1e-12
    for pre in ("", "ref_", "cross_"):
        for kind in ("mean", "rms"):
            key = f"{pre}{kind}_pairwise_rmsd"
            gates[key] = rm + (3 * L + 2) * EPS32 / 2 * ref_out[key] + 1e-12
    for key in ("emd_mean", "emd_var", "emd_total"):
        gates[key] = rm + 1e-7
    if "pca_w2_ref" in ref_out:
        ca_x, ca_r = aux["ca"]
        e = 2 * np.sqrt(3.0 * L) * g
        for key, data in (("pca_w2_ref", ca_r), ("pca_w2_joint", np.concatenate([ca_r, ca_x], 0))):
            fit = pca_fit(data)
            lam = fit["eigenvalues"]
            dC = 2 * np.sqrt(lam[0]) * e + e * e
            gap = min(lam[0] - lam[1], lam[1] - lam[2])
            ymax = max(np.linalg.norm(np.asarray(c).reshape(len(c), -1) - fit["mean"], axis=1).max() for c in (ca_x, ca_r))
            point = e + ymax * 2 * dC / gap
            gates[key] = 2 * np.sqrt(2.0) * point + 1e-9
            if key == "pca_w2_ref":
                S = lam.sum()
                dS = 2 * np.sqrt(S) * e + e * e
                gates["pca_explained"] = (dC + lam[:2] * dS / S) / S + 1e-12
    return gates
