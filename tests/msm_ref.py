"""NumPy fp64 restatement of csrc/k_msm.hip and of the chain around it (mdgen_amd/analysis.py kmeans_fit, msm_entries), the cases
of tests/test_msm_cpu.py and tests/test_msm_gpu.py, and their gates.

Distances.  dist2(x, c) = sum_j (x_j - c_j)^2 of the fp32 values in fp64.  The kernel forms the fp32 difference (relative error
eps32 / 2), squares it and adds d terms with fp32 FMAs: its error is below (d + 2) eps32 sum_j (|x_j| + |c_j|)^2.  With the maximum
over the centres this is gate_t, one number per point; `dist2` must be within gate_t of fp64.
Decided points.  Two candidate centres whose fp64 distances differ by more than 2 gate_t cannot change order in fp32: the point is
*decided* and must get the fp64 argmin.  The share of undecided points of a case is bounded by UNDECIDED_CAP; the restatement's own
share on every case is asserted on the CPU.
Sums.  The device adds fp32 values in fp64 in its own fixed order: any order is within 1e-12 sum |terms| of any other for fewer
than 2^20 terms (n eps64 < 1e-12 / 8), so sums and cost are compared with fp64 recomputed from the device's own assignment with
SUM_RTOL sum |terms|; counts are exact; the new centres are fp32(sums / counts) of the device's own sums, bit for bit.
k-means++.  The next index is recomputed from the fp64 cumulative sum of the device's own mind2; the comparison means something only
where the target u total is not within rounding of an interval end: the test asserts a margin of PP_MARGIN of the chosen element's
mass on both sides, which every case here has (asserted on the CPU for the restatement's mind2)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EPS32 = float(np.finfo(np.float32).eps)
UNDECIDED_CAP = 0.01
SUM_RTOL = 1e-12
PP_MARGIN = 1e-6
PP_SEED = 137

ASSIGN_CASES = [(1, 1, 1, 21), (63, 1, 2, 22), (64, 2, 2, 26), (65, 2, 3, 27), (257, 5, 3, 23), (4099, 2, 8, 11), (4099, 4, 100, 14),
                (4099, 34, 100, 28), (4099, 128, 256, 24), (100003, 3, 16, 25)]           # (n, d, k, seed)
PP_CASES = [(65, 1, 2, 22), (257, 5, 3, 23), (4099, 2, 8, 11), (4099, 4, 100, 14), (4099, 128, 256, 24), (100003, 3, 16, 25)]
BLOB_CASES = [(4099, 3, 5, 1), (4099, 2, 8, 2), (257, 5, 3, 3), (4099, 16, 100, 4)]
CLOUD_CASE = (4099, 2, 8, 11)
_NS, _KS = (1, 2, 65, 4099, 100003), (1, 2, 10, 100, 256)
COUNT_CASES = [(1, 0, 1), (1, 1, 2), (2, 1, 2), (2, 5, 10), (65, 0, 10), (65, 64, 100), (65, 65, 2), (65, 68, 256), (4099, 5, 100),
               (4099, 1, 256), (4099, 4098, 10), (100003, 5, 100), (100003, 1, 256)]      # (n, lag, k)
assert all(n in _NS and k in _KS and lag in (0, 1, 5, n - 1, n, n + 3) for n, lag, k in COUNT_CASES)


def inputs(n, d, k, seed):
    """x (n, d) fp32 standard normal and k of its rows as centres, drawn by the same generator."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, d)).astype(np.float32)
    return x, x[g.choice(n, size=k, replace=False)].copy()


def blobs(n, d, k, seed):
    """Well separated clusters: centres integers(-3, 4) * 10 (distinct rows), sigma 0.5, labels arange(n) % k."""
    g = np.random.default_rng(seed)
    while True:
        c = g.integers(-3, 4, size=(k, d)) * 10.0
        if len(np.unique(c, axis=0)) == k:
            break
    return (c[np.arange(n) % k] + 0.5 * g.standard_normal((n, d))).astype(np.float32)


# ---- distances and assignment ----------------------------------------------------------------------------------------
def dist2(x, centers):
    """fp64 [n, k]."""
    x64, c64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(centers, np.float32).astype(np.float64)
    out = np.empty((x64.shape[0], c64.shape[0]))
    for c in range(c64.shape[0]):
        out[:, c] = ((x64 - c64[c]) ** 2).sum(1)
    return out


def gate(x, centers):
    """gate_t [n] of the module docstring."""
    ax, ac = np.abs(np.asarray(x, np.float32).astype(np.float64)), np.abs(np.asarray(centers, np.float32).astype(np.float64))
    worst = np.zeros(ax.shape[0])
    for c in range(ac.shape[0]):
        worst = np.maximum(worst, ((ax + ac[c]) ** 2).sum(1))
    return (x.shape[1] + 2) * EPS32 * worst


def assign(x, centers):
    """(argmin [n] (lowest index on ties), the fp64 distance to it [n], decided [n] bool, gate_t [n])."""
    D = dist2(x, centers)
    arg = np.argmin(D, axis=1)
    g = gate(x, centers)
    if D.shape[1] == 1:
        return arg, D[:, 0], np.ones(len(D), bool), g
    two = np.partition(D, 1, axis=1)[:, :2]
    return arg, two[:, 0], (two[:, 1] - two[:, 0]) > 2.0 * g, g


def cluster_sums(x, arg, k):
    """(sums fp64 [k, d], sum of |terms| [k, d], counts int64 [k]) of the fp32 rows by cluster."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    sums, mags = np.zeros((k, x64.shape[1])), np.zeros((k, x64.shape[1]))
    np.add.at(sums, arg, x64)
    np.add.at(mags, arg, np.abs(x64))
    return sums, mags, np.bincount(arg, minlength=k).astype(np.int64)


def lloyd(x, centers0, max_iter=100, tol=1e-5):
    """The iteration of `kmeans_fit` in fp64 on fp32 centres: assign, cost, centres <- fp32(sums / counts) (an empty cluster keeps
    its centre), stop after the step with |cost_prev - cost| <= tol cost (never the first).
    {"centers" fp32, "assign" (the last step's), "steps", "cost_history", "undecided" (points, summed over the steps)}."""
    c = np.array(centers0, np.float32)
    k = c.shape[0]
    hist, undecided = [], 0
    arg = np.zeros(len(x), np.int64)
    for step in range(max_iter):
        arg, dmin, decided, _ = assign(x, c)
        undecided += int((~decided).sum())
        hist.append(float(dmin.sum()))
        sums, _, counts = cluster_sums(x, arg, k)
        live = counts > 0
        c = c.copy()
        c[live] = (sums[live] / counts[live, None]).astype(np.float32)
        if step >= 1 and abs(hist[-2] - hist[-1]) <= tol * hist[-1]:
            break
    return {"centers": c, "assign": arg, "steps": len(hist), "cost_history": np.array(hist), "undecided": undecided}


# ---- k-means++ -------------------------------------------------------------------------------------------------------
def pp_next(mind2, u, n):
    """(index, margin) of a round from its mind2 values: the smallest i with cumsum_i > u total in fp64 (floor(u n) when the total is
    zero: margin inf); margin = the target's distance to the nearer end of the chosen interval, in units of the element's mass."""
    w = np.asarray(mind2, np.float32).astype(np.float64)
    cum = np.cumsum(w)
    total = cum[-1]
    if not total > 0:
        return min(int(np.floor(u * n)), n - 1), np.inf
    target = u * total
    i = int(np.searchsorted(cum, target, side="right"))
    lo = cum[i - 1] if i else 0.0
    return i, min(target - lo, cum[i] - target) / w[i]


def pp(x, u):
    """k-means++ of the header in fp64: (chosen int64 [k], the smallest margin of the rounds)."""
    n, k = x.shape[0], len(u)
    x64 = np.asarray(x, np.float32).astype(np.float64)
    chosen = np.zeros(k, np.int64)
    chosen[0] = min(int(np.floor(u[0] * n)), n - 1)
    mind2 = np.full(n, np.inf)
    margin = np.inf
    for r in range(1, k):
        mind2 = np.minimum(mind2, ((x64 - x64[chosen[r - 1]]) ** 2).sum(1))
        chosen[r], m = pp_next(mind2.astype(np.float32), u[r], n)
        margin = min(margin, m)
    return chosen, margin


def fit(x, k, max_iter=100, tol=1e-5, seed=137):
    """`kmeans_fit` restated: default_rng(seed).random(k) -> `pp` -> `lloyd`."""
    chosen, _ = pp(x, np.random.default_rng(seed).random(k))
    return lloyd(x, np.asarray(x, np.float32)[chosen], max_iter, tol)


# ---- counts ----------------------------------------------------------------------------------------------------------
def dtraj_case(n, lag, k):
    """A dtraj of n states in -1 .. k (both ends are outside and dropped), sticky so that the counts are uneven."""
    g = np.random.default_rng(n * 1000 + lag * 10 + k)
    d = g.integers(-1, k + 1, size=n)
    hold = g.random(n) < 0.6
    for t in range(1, n):
        if hold[t]:
            d[t] = d[t - 1]
    return d.astype(np.int32)


def count_matrix(dtraj, lag, k):
    """(counts int64 [k, k], dropped) by np.add.at."""
    d = np.asarray(dtraj, np.int64)
    C = np.zeros((k, k), np.int64)
    if lag >= len(d):
        return C, 0
    a, b = d[:len(d) - lag], d[lag:]
    ok = (a >= 0) & (a < k) & (b >= 0) & (b < k)
    np.add.at(C, (a[ok], b[ok]), 1)
    return C, int((~ok).sum())


# ---- Markov chains for the host estimators ---------------------------------------------------------------------------
def three_well_chain(steps=200000, seed=0, states=30):
    """A dtraj of a nearest-neighbour walk on `states` states in a three-well potential (reversible by construction)."""
    g = np.random.default_rng(seed)
    s = np.arange(states)
    energy = 2.0 * np.cos(2 * np.pi * 3 * s / states)
    d = np.empty(steps, np.int64)
    cur = states // 6
    moves, uni = g.integers(0, 2, size=steps) * 2 - 1, g.random(steps)
    for t in range(steps):
        nxt = cur + moves[t]
        if 0 <= nxt < states and uni[t] < min(1.0, np.exp(energy[cur] - energy[nxt])):
            cur = nxt
        d[t] = cur
    return d


def block_chain(sizes=(4, 5, 3), eps=1e-3):
    """(T, pi, blocks): a reversible chain of dense blocks with transition weight eps between them."""
    k = sum(sizes)
    g = np.random.default_rng(5)
    W = np.full((k, k), eps)
    blocks, o = [], 0
    for sz in sizes:
        a = g.random((sz, sz)) + 0.5
        W[o:o + sz, o:o + sz] = a + a.T
        blocks.append(np.arange(o, o + sz))
        o += sz
    return W / W.sum(1, keepdims=True), W.sum(1) / W.sum(), blocks


# ---- end to end ------------------------------------------------------------------------------------------------------
E2E = dict(seq="FLRH", F_ref=6000, F_traj=3000, seed_ref=22, seed_traj=21, walk=0.2, tica_lag=5, msm_k=12, msm_states=3, md_msm_lag=5,
           msm_lag=2, kmeans_seed=137)


def e2e_trajectories():
    import analysis_ref as R
    aat = R.aatype_of(E2E["seq"])
    return (aat, R.peptide(E2E["F_traj"], aat, seed=E2E["seed_traj"], walk=E2E["walk"]),
            R.peptide(E2E["F_ref"], aat, seed=E2E["seed_ref"], walk=E2E["walk"]))


def e2e_restatement():
    """The whole chain on the CPU in fp64 (torsions, tICA, projection at the model's dim rounded to fp32, `fit`, discretisation):
    (d_ref, d_traj, the fit) for `host_chain`."""
    import analysis_ref as R
    import tica_ref as T
    from mdgen_amd.analysis import torsion_features
    aat, traj, ref = e2e_trajectories()
    _, quad = torsion_features(aat)
    a_ref, a_traj = R.dihedrals(ref, quad).astype(np.float32), R.dihedrals(traj, quad).astype(np.float32)
    lag = E2E["tica_lag"]
    model = T.solve(len(a_ref) - lag, *T.moments(a_ref, lag))
    W = model["W"][:, :model["dim"]]
    y_ref, y_traj = (T.transform(a, model["mean"], W).astype(np.float32) for a in (a_ref, a_traj))
    km = fit(y_ref, E2E["msm_k"], seed=E2E["kmeans_seed"])
    return assign(y_ref, km["centers"])[0], assign(y_traj, km["centers"])[0], km


def host_chain(d_ref, d_traj, k, nstates, md_lag, traj_lag):
    """The host part of `msm_entries` from the two microstate dtrajs, with NumPy counts: the dict of its array-valued entries."""
    from mdgen_amd import msm as M
    C, _ = count_matrix(d_ref, md_lag, k)
    model = M.estimate_msm(C, md_lag)
    assert len(model["active_set"]) == k
    pc = M.pcca(model["transition_matrix"], model["pi"], nstates)
    meta = pc["metastable_assignments"]
    l_ref, l_traj = meta[np.asarray(d_ref, np.int64)], meta[np.asarray(d_traj, np.int64)]
    cmsm = M.estimate_msm(count_matrix(l_ref, md_lag, nstates)[0], md_lag)         # (a second pass: must equal the lumped matrix)
    tm = M.estimate_msm(count_matrix(l_traj, traj_lag, nstates)[0], traj_lag)
    eye, zero = np.eye(nstates), np.zeros(nstates)

    def filled(m, base, key):
        out = base.copy()
        if out.ndim == 2:
            for a, i in enumerate(m["active_set"]):
                for b, j in enumerate(m["active_set"]):
                    out[i, j] = m[key][a, b]
        else:
            out[m["active_set"]] = m[key]
        return out
    return {"msm": model, "pcca": pc, "cmsm": cmsm, "traj_msm": tm,
            "traj_metastable_probs": (l_traj == np.arange(nstates)[:, None]).mean(1),
            "ref_metastable_probs": (l_ref == np.arange(nstates)[:, None]).mean(1),
            "msm_transition_matrix": filled(cmsm, eye, "transition_matrix"), "pcca_pi": pc["pi_coarse"],
            "msm_pi": filled(cmsm, zero, "pi"), "traj_transition_matrix": filled(tm, eye, "transition_matrix"),
            "traj_pi": filled(tm, zero, "pi")}
