"""NumPy fp64 restatement of csrc/k_tps.hip (mdgen_tp_sample, include/mdgen_amd.h) and of the reference's transition-path
estimators, for tests/test_tps_cpu.py and tests/test_tps_gpu.py.

The sampler.  Every operation of the draw is one rounded fp64 operation in a stated order -- the products Ta[a][j] Ba[N-t-1][j], the
running sum over j ascending (`np.cumsum` adds sequentially), the product u c_{k-1}, the comparison -- and the uniform is exact, so
the device's paths must equal `sample`'s to the last state: the GPU test asserts equality, not closeness.
The likelihood.  `likelihood_loop` is the reference's `get_tp_likelihood` with its two `matrix_power` calls per step; the project's
`msm.tp_likelihood` forms the same powers by repeated products, which differ by rounding: k eps64 per product, at most N - 1 = 100 of
them, 1e-12 with a margin of 100 at k = 10.
Exact values.  `enumerate_bridge` walks all k^(N-2) bridge paths; `msm.bridge_exact` must agree at 1e-12.
Monte-Carlo bounds (test_tps_cpu.py): a per-path state fraction and a per-path validity flag lie in [0, 1], so their standard
deviation is at most 1/2 and the mean of n paths has a standard error of at most 1 / (2 sqrt n); the gate is five of those."""
import itertools

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: counter words (uint64 arrays holding 32-bit values, broadcastable) under two key words -> four uint64 arrays."""
    c = [np.asarray(v, np.uint64) & _MASK for v in (c0, c1, c2, c3)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniform(seed, stream, sample, t):
    """u = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 at the counter (sample low, sample high, t, stream), key {seed low, seed high}."""
    seed = int(seed) % (1 << 64)
    sample = np.asarray(sample, np.uint64)
    x = philox(sample & _MASK, sample >> np.uint64(32), np.uint64(int(t)), np.uint64(int(stream) % (1 << 32)), seed & 0xFFFFFFFF,
               seed >> 32)
    return (((x[0] >> np.uint64(5)) << np.uint64(26)) + (x[1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def bridge_table(T, end, N):
    """B[m] = matrix_power(T, m)[:, end], as the reference evaluates it."""
    return np.stack([np.linalg.matrix_power(np.asarray(T, np.float64), m)[:, end] for m in range(N)])


def sample(Ta, Ba, start, end, n_samples, seed, stream, sample_base=0):
    """paths int64 [n_samples, N] by the header's draw rule, vectorised over the paths (the steps of a path are sequential).
    A path whose weights sum to zero (or NaN) at step t holds -1 from t on."""
    Ta, Ba = np.asarray(Ta, np.float64), np.asarray(Ba, np.float64)
    N, k = Ba.shape
    ids = (np.arange(n_samples, dtype=np.uint64) + np.uint64(int(sample_base) % (1 << 64)))
    paths = np.full((n_samples, N), -1, np.int64)
    paths[:, 0] = start
    live = np.ones(n_samples, bool)
    a = np.full(n_samples, start, np.int64)
    for t in range(1, N - 1):
        w = Ta[a] * Ba[N - t - 1][None, :]
        c = np.cumsum(w, axis=1)
        total = c[:, -1]
        live &= total > 0
        target = uniform(seed, stream, ids, t) * total
        over = c > target[:, None]
        first = np.argmax(over, axis=1)
        last_pos = k - 1 - np.argmax((w > 0)[:, ::-1], axis=1)
        a = np.where(live, np.where(over.any(1), first, last_pos), 0)
        paths[live, t] = a[live]
    paths[live, N - 1] = end
    return paths


def likelihood_loop(paths, T):
    """The quantity of the reference's get_tp_likelihood (mdgen/analysis.py:79-95) in its loop form: at every step the two matrix
    powers are formed afresh with `matrix_power`, the end state is the FIRST path's last state, NaN becomes 0.  fp64 [P, N - 1]."""
    paths, T = np.asarray(paths, np.int64), np.asarray(T, np.float64)
    N = paths.shape[1]
    end = paths[0, -1]
    out = np.empty((paths.shape[0], N - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, N):
            a, b = paths[:, t - 1], paths[:, t]
            to_go, to_go_before = np.linalg.matrix_power(T, N - t - 1), np.linalg.matrix_power(T, N - t)
            out[:, t - 1] = to_go[b, end] * T[a, b] / to_go_before[a, end]
    out[np.isnan(out)] = 0
    return out


def state_probs_loop(tp, num_states=10):
    counts = np.zeros(num_states)
    for s in np.asarray(tp).reshape(-1):
        counts[s] += 1
    return counts / counts.sum()


def enumerate_bridge(Ta, start, end, N, Tb=None, phi=None):
    """All k^(N-2) bridge paths: {"Z", "occupancy"} and, with Tb and phi, {"prob", "valid_rate", "valid_prob"}: the expectations
    under the bridge measure prod Ta / Z of the state fractions, of likelihood_loop(phi(path), Tb).prod() and of its positivity."""
    Ta = np.asarray(Ta, np.float64)
    k = Ta.shape[0]
    Z, occ, prob, valid = 0.0, np.zeros(k), 0.0, 0.0
    for mid in itertools.product(range(k), repeat=N - 2):
        path = np.array((start,) + mid + (end,))
        p = float(np.prod(Ta[path[:-1], path[1:]]))
        if p == 0:
            continue
        Z += p
        occ += p * np.bincount(path, minlength=k) / N
        if Tb is not None:
            like = float(likelihood_loop(np.asarray(phi)[path][None, :], Tb).prod())
            prob += p * like
            valid += p * (like > 0)
    out = {"Z": Z, "occupancy": occ / Z}
    if Tb is not None:
        out.update(prob=prob / Z, valid_rate=valid / Z, valid_prob=prob / valid if valid > 0 else float("nan"))
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------
def chain(k, seed, zero_share=0.0, lazy=0.0):
    """A row-stochastic fp64 [k, k] matrix: uniform weights, a share of the off-diagonal entries set to zero (the diagonal stays
    positive, so every state can wait), `lazy` added to the diagonal before the rows are normalised."""
    g = np.random.default_rng(seed)
    W = g.random((k, k)) + 0.05
    W[(g.random((k, k)) < zero_share) & ~np.eye(k, dtype=bool)] = 0.0
    W += lazy * np.eye(k)
    return W / W.sum(1, keepdims=True)


PATH_CASES = [(1, 2, 1, 0.0), (1, 3, 2, 0.0), (257, 11, 10, 1 / 3), (4099, 11, 10, 1 / 3), (1000, 101, 10, 0.0), (65, 11, 64, 0.0)]
#            (n_samples, N, k, share of Ta that is zero)


def path_case(n, N, k, zero_share):
    """(Ta, start, end) of a PATH_CASES row; the end is reachable (asserted by the CPU test for every row)."""
    Ta = chain(k, 1000 * k + N, zero_share)
    return Ta, 0, k - 1


def score_case(k=10, kb=7, seed=10):
    """(Tb, phi): a scoring chain with zeros (10 of its 49 entries) and a map that is neither the identity nor one to one.  Under it
    62 % of the (4099, 11, 10) case's paths and 2 % of the (1000, 101, 10) case's have a positive likelihood."""
    g = np.random.default_rng(seed)
    phi = g.integers(0, kb, size=k).astype(np.int32)
    phi[0], phi[k - 1] = 0, kb - 1
    return chain(kb, seed + 1, 0.15), phi


STAT_CASE = dict(k=6, N=11, n=40000, seed_a=11, zero_a=0.2, seed_b=16, zero_b=0.15, phi=(2, 0, 1, 4, 5, 3), start=0, end=5, seed=137,
                 stream=3)      # the exact valid rate is 0.454 (asserted to lie in 0.2 .. 0.8 by the CPU test)
