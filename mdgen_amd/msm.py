"""Markov-state-model estimators on k x k matrices (k <= 256), in NumPy fp64 on the host: the connected set, the reversible
maximum-likelihood transition matrix, PCCA+ lumping and the reference's choice of a start / end state.  They restate what the
reference (mdgen/analysis.py get_msm, scripts/analyze_peptide_sim.py:153-197, tps_inference.py:110-112) asks of pyemma's
`estimate_markov_model(dtraj, lag)` (defaults: reversible, sliding count, largest connected set) and `msm.pcca(m)`; every rule is
stated in the docstrings below.  pyemma is not installed where this was written: agreement with it is unverified.  The count matrix
itself, and k-means before it, are the device's (mdgen_amd/analysis.py count_matrix, kmeans_fit; csrc/k_msm.hip).

Left out on purpose: pyemma refines the PCCA+ transformation with a Nelder-Mead search after the inner simplex algorithm -- here the
inner simplex result is final; Bayesian / HMM estimators, error bars, plots.

The transition-path estimators of the reference's mdgen/analysis.py and tps_inference.py:110-127 are here too (`bridge_table`,
`tp_likelihood`, `state_probs`, `bridge_exact`, `tps_endpoints`); the bridge paths themselves are sampled on the device
(mdgen_amd/analysis.py tp_sample; csrc/k_tps.hip).

Imports without torch or scipy.  Estimator results are plain dicts of NumPy arrays and ints."""
from __future__ import annotations

import numpy as np


def largest_connected_set(C):
    """Sorted int64 indices of the largest strongly connected component of the directed graph i -> j where C[i, j] > 0 (every
    state reaches itself).  Reachability is the boolean closure of (C > 0) | I by repeated squaring; two components of the same
    size: the one that contains the lowest state."""
    C = np.asarray(C)
    k = C.shape[0]
    if C.ndim != 2 or C.shape[1] != k or k < 1:
        raise ValueError(f"count matrix {C.shape}: expected [k, k], k >= 1")
    reach = (C > 0) | np.eye(k, dtype=bool)
    hops = 1
    while hops < k:
        reach = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        hops *= 2
    both = reach & reach.T
    best = both[0]
    for i in range(1, k):
        if both[i].sum() > best.sum():      # (strictly: the earlier, lower component wins a tie)
            best = both[i]
    return np.flatnonzero(best).astype(np.int64)


def mle_reversible(C, maxerr=1e-8, maxiter=1_000_000):
    """(T, pi, iterations): the reversible maximum-likelihood transition matrix of a count matrix C on a connected set, by the
    dense fixed-point iteration

      S = C + C',  c_i = sum_j C_ij,  X = S / sum S;
      x_i = sum_j X_ij;  X_ij <- S_ij / (c_i / x_i + c_j / x_j), renormalised to sum 1;  x_i' = sum_j X_ij;
      stop when max_i |x_i' - x_i| / ((x_i' + x_i) / 2) < maxerr;
      T_ij = X_ij / x_i,  pi = x / sum x.

    T satisfies detailed balance with pi by construction (X is symmetric).  ValueError for a state without counts (it is in no
    connected set of more than one state) and when `maxiter` iterations do not converge."""
    C = np.asarray(C, np.float64)
    k = C.shape[0]
    if C.ndim != 2 or C.shape[1] != k or k < 1:
        raise ValueError(f"count matrix {C.shape}: expected [k, k], k >= 1")
    if k == 1:
        return np.ones((1, 1)), np.ones(1), 0
    S = C + C.T
    c = C.sum(1)
    if not (c > 0).all() or not (S.sum(1) > 0).all():
        raise ValueError("a state of the count matrix has no counts: restrict it to its connected set first")
    X = S / S.sum()
    x = X.sum(1)
    for it in range(1, int(maxiter) + 1):
        q = c / x
        X = S / (q[:, None] + q[None, :])
        X /= X.sum()
        xn = X.sum(1)
        err = np.max(np.abs(xn - x) / ((xn + x) / 2.0))
        x = xn
        if err < maxerr:
            return X / x[:, None], x / x.sum(), it
    raise ValueError(f"the reversible estimator did not converge in {int(maxiter)} iterations (error {err:.3e} >= {maxerr:g})")


def estimate_msm(C_full, lag, maxerr=1e-8, maxiter=1_000_000):
    """What `pyemma.msm.estimate_markov_model(dtraj, lag)` holds, from the full count matrix of the dtraj at that lag:
    {"lag", "active_set" (`largest_connected_set`), "count_matrix" (restricted to it, int64 when C_full is), "transition_matrix",
    "pi"} (`mle_reversible`)."""
    C_full = np.asarray(C_full)
    active = largest_connected_set(C_full)
    Ca = np.ascontiguousarray(C_full[np.ix_(active, active)])
    T, pi, _ = mle_reversible(Ca, maxerr, maxiter)
    return {"lag": int(lag), "active_set": active, "count_matrix": Ca, "transition_matrix": T, "pi": pi}


def _inner_simplex(V):
    """Rows of V [k, m] that span the simplex: the row of largest norm; that row subtracted from all; then, m - 1 times: the rows
    made orthogonal to the previous pick (Gram-Schmidt), the row of largest norm picked, all rows scaled by that norm.  The first
    row wins a tie."""
    k, m = V.shape
    idx = np.zeros(m, np.int64)
    idx[0] = int(np.argmax(np.linalg.norm(V, axis=1)))
    O = V - V[idx[0]]
    for j in range(1, m):
        t = O[idx[j - 1]].copy()              # (j = 1: the zero row, nothing to project out)
        O = O - np.outer(O @ t, t)
        norms = np.linalg.norm(O, axis=1)
        idx[j] = int(np.argmax(norms))
        if not norms[idx[j]] > 0:
            raise ValueError(f"PCCA+: the {m} eigenvectors span fewer than {m} dimensions")
        O = O / norms[idx[j]]
    return idx


def pcca(T, pi, m):
    """PCCA+ lumping of a reversible transition matrix T with stationary distribution pi into m metastable sets:

      1. Ts = diag(sqrt pi) T diag(1 / sqrt pi), symmetrised;  2. `eigh`, the m largest eigenvalues, descending;
      3. right eigenvectors V = u / sqrt(pi) (so that sum_i pi_i V_ij^2 = 1); column 0 is set to all ones, in every other
         column the entry of largest magnitude is made positive (the first such entry on ties);
      4. the inner simplex algorithm (`_inner_simplex`) picks m rows idx;  A = inv(V[idx]),  chi = V A;
      5. chi clipped to [0, 1], rows renormalised to sum 1.

    {"memberships" chi [k, m], "metastable_assignments" argmax over each row (int64), "pi_coarse" = pi chi, "eigenvalues" [m]}.
    pyemma's Nelder-Mead refinement of A is left out (module docstring): raw memberships can leave [0, 1], hence step 5."""
    T = np.asarray(T, np.float64)
    pi = np.asarray(pi, np.float64).ravel()
    k, m = T.shape[0], int(m)
    if T.shape != (k, k) or pi.shape[0] != k:
        raise ValueError(f"T {T.shape} / pi {pi.shape}: expected [k, k] and [k]")
    if not 1 <= m <= k:
        raise ValueError(f"PCCA+ into {m} sets needs 1 <= m <= {k} states")
    if not (pi > 0).all():
        raise ValueError("PCCA+ needs a positive stationary distribution")
    sq = np.sqrt(pi)
    Ts = sq[:, None] * T / sq[None, :]
    lam, u = np.linalg.eigh((Ts + Ts.T) / 2.0)
    lam, u = lam[::-1][:m].copy(), u[:, ::-1][:, :m]
    V = u / sq[:, None]
    big = np.argmax(np.abs(V), axis=0)
    V = V * np.where(V[big, np.arange(m)] < 0, -1.0, 1.0)
    V[:, 0] = 1.0
    if m == 1:
        chi = np.ones((k, 1))
    else:
        idx = _inner_simplex(V)
        chi = V @ np.linalg.inv(V[idx])
    chi = np.clip(chi, 0.0, 1.0)
    chi = chi / chi.sum(1, keepdims=True)
    return {"memberships": chi, "metastable_assignments": np.argmax(chi, axis=1).astype(np.int64), "pi_coarse": pi @ chi,
            "eigenvalues": lam}


def least_flux_pair(cmsm):
    """(start_state, end_state) as the reference's tps_inference.py:110-112 picks them from the coarse MSM: the argmin (first in
    row-major order) of transition_matrix * pi[None, :] with entries below 1e-7 set to inf, mapped through `active_set` to
    metastable-state numbers."""
    flux = np.array(cmsm["transition_matrix"], np.float64) * np.asarray(cmsm["pi"], np.float64)[None, :]
    flux[flux < 1e-7] = np.inf
    a, b = np.unravel_index(int(np.argmin(flux)), flux.shape)
    active = np.asarray(cmsm["active_set"])
    return int(active[a]), int(active[b])


# ---- transition paths ------------------------------------------------------------------------------------------------
# A path of length N of a chain T pinned at both ends (a Markov bridge) leaves state a at step t = 1 .. N - 1 for state b with
# probability T[a, b] B[N - t - 1][b] / B[N - t][a], B[m][i] = (T^m)[i, end]: the reference's `sample_tp` and `get_tp_likelihood`
# (mdgen/analysis.py:61-95), which evaluate both powers with `np.linalg.matrix_power` at every step.
def bridge_table(T, end, N):
    """B fp64 [N, k]: B[0] = e_end, B[m] = T @ B[m - 1], so B[m][i] = (T^m)[i, end] -- the reference's
    `matrix_power(T, m)[:, end]` up to rounding."""
    T = np.asarray(T, np.float64)
    k, N, end = T.shape[0], int(N), int(end)
    if T.ndim != 2 or T.shape[1] != k or k < 1:
        raise ValueError(f"transition matrix {T.shape}: expected [k, k], k >= 1")
    if N < 1 or not 0 <= end < k:
        raise ValueError(f"bridge table of {N} rows to state {end} of {k}")
    B = np.zeros((N, k))
    B[0, end] = 1.0
    for m in range(1, N):
        B[m] = T @ B[m - 1]
    return B


def tp_likelihood(tp, T):
    """fp64 [P, N - 1]: the reference's `get_tp_likelihood(tp, T)`, literally.  With s_N = tp[0, -1] -- the FIRST path's last
    state, for every path -- and B = bridge_table(T, s_N, N), step t = i + 1 has probability T[a, b] B[N - t - 1][b] / B[N - t][a],
    a = tp[:, i], b = tp[:, i + 1]; NaN (0 / 0: a state that cannot reach s_N) becomes 0."""
    tp = np.asarray(tp, np.int64)
    T = np.asarray(T, np.float64)
    if tp.ndim != 2 or tp.shape[0] < 1 or tp.shape[1] < 2:
        raise ValueError(f"paths {tp.shape}: expected [P, N], P >= 1, N >= 2")
    N = tp.shape[1]
    B = bridge_table(T, int(tp[0, -1]), N)
    out = np.empty((tp.shape[0], N - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(N - 1):
            t = i + 1
            a, b = tp[:, i], tp[:, i + 1]
            out[:, i] = T[a, b] * B[N - t - 1][b] / B[N - t][a]
    out[np.isnan(out)] = 0
    return out


def state_probs(tp, num_states=10):
    """The reference's `get_state_probs`: bincount(tp, minlength=num_states) / its sum."""
    counts = np.bincount(np.asarray(tp, np.int64).reshape(-1), minlength=int(num_states))
    return counts / counts.sum()


def bridge_exact(Ta, start, end, N, Tb=None, phi=None):
    """The exact expectations that the reference estimates from 1000 sampled bridge paths of Ta (length N, start -> end):

      Z_a = (Ta^(N-1))[start, end];   "occupancy"[j] = (1 / N) sum_{t=0}^{N-1} (Ta^t)[start, j] (Ta^(N-1-t))[j, end] / Z_a,
      the expected share of a path's N frames spent in state j (what `state_probs` of the sampled paths estimates).

    With a scoring matrix Tb and the index map phi from Ta's states into Tb's (identity when None), Tb'[i, j] = Tb[phi i, phi j],
    Z_b = (Tb^(N-1))[phi start, phi end], o the elementwise product:

      "prob" = ((Ta o Tb')^(N-1))[start, end] / (Z_a Z_b)     the mean of `tp_likelihood(phi(paths), Tb).prod(-1)` (0 when Z_b = 0)
      "valid_rate" = ((Ta o [Tb' > 0])^(N-1))[start, end] / Z_a     the share of paths with a positive product
      "valid_prob" = prob / valid_rate                        the mean over those (NaN when there are none)

    {"Z", "occupancy"} and, with Tb, {"prob", "valid_rate", "valid_prob"}.  ValueError when Z_a = 0."""
    Ta = np.asarray(Ta, np.float64)
    k, N, start, end = Ta.shape[0], int(N), int(start), int(end)
    if Ta.ndim != 2 or Ta.shape[1] != k or N < 2 or not (0 <= start < k and 0 <= end < k):
        raise ValueError(f"bridge of length {N} from {start} to {end} on {Ta.shape}")

    def forward(M):      # F[t] = e_start' M^t
        F = np.zeros((N, k))
        F[0, start] = 1.0
        for t in range(1, N):
            F[t] = F[t - 1] @ M
        return F
    Fa, Ba = forward(Ta), bridge_table(Ta, end, N)
    Z = float(Ba[N - 1, start])
    if not Z > 0:
        raise ValueError(f"end state not reachable in N - 1 steps: (Ta^{N - 1})[{start}, {end}] = {Z}")
    out = {"Z": Z, "occupancy": (Fa * Ba[::-1]).sum(0) / (N * Z)}
    if Tb is not None:
        Tb = np.asarray(Tb, np.float64)
        phi = np.arange(k) if phi is None else np.asarray(phi, np.int64)
        if phi.shape != (k,) or phi.min() < 0 or phi.max() >= Tb.shape[0]:
            raise ValueError(f"phi {phi.shape}: expected {k} indices into {Tb.shape[0]} states")
        Tbp = Tb[np.ix_(phi, phi)]
        Zb = float(bridge_table(Tb, int(phi[end]), N)[N - 1, int(phi[start])])
        valid = float(forward(Ta * (Tbp > 0))[N - 1, end]) / Z
        prob = float(forward(Ta * Tbp)[N - 1, end]) / (Z * Zb) if Zb > 0 else 0.0
        out.update(prob=prob, valid_rate=valid, valid_prob=prob / valid if valid > 0 else float("nan"))
    return out


def tps_endpoints(cmsm, meta, ref_dtraj, n_paths, seed, stream):
    """(start_state, end_state, start_idx int64 [n_paths], end_idx int64 [n_paths]) as the reference's tps_inference.py:110-127
    chooses them: the states are `least_flux_pair(cmsm)`; ref_discrete = meta[ref_dtraj] (the MD trajectory's metastable states);
    every path draws one frame of the start state and one of the end state.  rng = np.random.default_rng([seed, stream]); per
    path, in order, start_idxs[rng.integers(len(start_idxs))] and then end_idxs[rng.integers(len(end_idxs))].  (The reference draws
    from NumPy's unseeded global state: the frames here are reproducible and not the reference's draw for draw.)  ValueError when
    the MD trajectory has no frame in either state -- the reference prints and skips the peptide."""
    start_state, end_state = least_flux_pair(cmsm)
    ref_discrete = np.asarray(meta, np.int64)[np.asarray(ref_dtraj, np.int64)]
    start_idxs, end_idxs = np.flatnonzero(ref_discrete == start_state), np.flatnonzero(ref_discrete == end_state)
    if len(start_idxs) == 0 or len(end_idxs) == 0:
        raise ValueError(f"no start or end state found: {len(start_idxs)} frames in state {start_state}, {len(end_idxs)} in "
                         f"state {end_state}")
    rng = np.random.default_rng([int(seed), int(stream)])
    si, ei = np.empty(int(n_paths), np.int64), np.empty(int(n_paths), np.int64)
    for p in range(int(n_paths)):
        si[p] = start_idxs[rng.integers(len(start_idxs))]
        ei[p] = end_idxs[rng.integers(len(end_idxs))]
    return start_state, end_state, si, ei
