"""Time of each leg of the trajectory analysis, device events around enqueued work, one JSON line per leg:

  dihedrals     `mdgen_traj_dihedrals`: F = 100 000 frames of a tetrapeptide, 16 torsions (and L = 8, 35 torsions)
  histograms    `mdgen_traj_histograms`: the 100-bin histograms of every torsion and two 50 x 50 ones, same F
  acov          `mdgen_traj_acov` at the sampler's size (n 1e5, K 1000, NF 25) and at the reference's MD size (n 1e6, K 1e5)
  fft           the same autocovariance through torch.fft on the same device (fp32, zero-padded to 2^ceil(log2(2 n))): for scale
  numpy         the same through np.fft on the host (fp64), sampler size only: what a script without the device would do
  moments       `mdgen_traj_lagged_moments`: n = 1e5 and 1e6 frames, NF 25 (D = 50 features), lag 1000
  project       `mdgen_traj_project`: n = 1e6, NF 25, d = 2 and d = 10
  series        `mdgen_traj_series_acov`: one series at the sampler's size (n 1e5, K 1000) and at the MD size (n 1e6, K 1e5)
  tica          `analyze(tica=True)` of one tetrapeptide, 1e5 sampled frames against 1e6 MD frames, beside `analyze()` without it
  kmeans_pp     `mdgen_traj_kmeans_pp`: all 100 rounds on n = 1e6 points of d = 10 components (the MD trajectory's tICA projection)
  kmeans_step   `mdgen_traj_kmeans_step`: one Lloyd iteration at the same size, k = 100; beside it `numpy_step_ms_1e5`, the same step in
                NumPy fp64 on the host at 1e5 points
  kmeans_fit    `kmeans_fit`: k-means++ and 100 step launches with the one read-back, wall time
  count_matrix  `mdgen_traj_count_matrix`: the 1e6-frame dtraj at lag 1000, k = 100 (LDS counters) and k = 256 (global ones)
  msm           `analyze(msm=True)` beside `analyze(tica=True)`, the same trajectories as `tica`; `host_ms`: the estimators alone
  tps           `mdgen_tp_sample` (10 states, scored under a second 10-state chain) at (n_samples, N) = (1000, 11) and (1e6, 101):
                the kernel alone (events), `tp_sample` with its tables' upload and the paths' copy back (wall), and `numpy_ms`, the
                vectorised NumPy restatement of tests/tps_ref.py with `msm.tp_likelihood` on the same box; then one
                `analyze_peptide_tps.analyze_tps` peptide at the reference's size: 1000 paths x 100 frames, a 1e6-frame replica,
                seven replica lengths (wall; `metadata_wall_ms`: `tps_inference.build_metadata` of the 1e6-frame MD trajectory)
  ensemble      the `mdgen_ens_*` kernels and `analyze_ensemble` at the ATLAS size -- 250 sampled frames against 30 003 MD frames of
                256 residues (3 584 atom14 slots, 256 C-alphas) -- and `mdgen_ens_superpose` at 1e6 frames x 56 atoms.  Beside
                `mdgen_ens_pairwise_d2` the plain torch expression on the same box: `torch.cdist` on [F, 3A] in chunks of 2 048
                rows with the same two fp64 sums, in its matrix-product mode (`torch_cdist_mm_ms`) and in its direct mode
                (`torch_cdist_direct_ms`); beside `mdgen_ens_contact_counts` a chunked torch comparison (512 frames at a time).
                `sasa_counts`: `mdgen_ens_sasa_counts` over the 250 and the 30 003 frames (P = 960, probe 2.8 A, Bondi radii, existing
                atoms by `atom14_mask`); beside each a chunked torch restatement of the same counts on the same box, run on the
                first `--sasa_torch_frames` frames only (it is far slower: `torch_ms_per_frame` against `ms_per_frame`) with the
                number of entries that differ there (torch need not fuse the multiply-adds: borderline points may differ).  Then
                `analyze_ensemble` without and with `sasa=True`.
                Not part of `--leg all` (it allocates 1.3 GB of coordinates).  `--leg sasa`: the `sasa_counts` records and the two
                `analyze_ensemble(pca=False)` wall times alone.

Beside each of the last four, `numpy_ms`: the same definition in NumPy fp64 on the host, the copy of the device array to the host
included (moments: cos / sin, three matrix products and two sums; project: cos / sin, the centred product; series: np.fft; tica:
the tICA entries -- moments, solver, two projections, four histograms, two autocovariances -- from the angles).

    python scripts/analysis_bench.py [--leg all|dihedrals|histograms|acov|fft|numpy|moments|project|series|tica|kmeans_pp|kmeans_step|kmeans_fit|
                                           count_matrix|msm|tps|ensemble|sasa] [--size sampler|md|both]
                                     [--reps 5] [--sasa_torch_frames 4]

acov reports multiply-adds (2 n' (K + 1) NF with n' the mean number of terms per lag) over time and that rate's share of the
fp32 vector peak (157.3 TFLOP/s = 78.6e12 multiply-adds / s)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"sampler": (100000, 1000, 25), "md": (1000000, 100000, 25)}
FMA_PEAK = 256 * 4 * 32 * 2.4e9


def timed_ms(fn, reps):
    """Best and median of `reps` event-timed calls after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def angles(n, NF, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.cumsum(0.2 * torch.randn(n, NF, generator=g), 0)
    return torch.atan2(torch.sin(x), torch.cos(x)).to(dev).contiguous()


def macs(n, K, NF):
    k = np.arange(K + 1, dtype=np.float64)
    return 2.0 * NF * float((n - k).sum())


def host_features(ang):
    """fp64 cos / sin features of a device angle tensor, interleaved: the copy to the host is part of what is timed."""
    a = ang.double().cpu().numpy()
    x = np.empty((a.shape[0], 2 * a.shape[1]))
    x[:, 0::2], x[:, 1::2] = np.cos(a), np.sin(a)
    return x


def host_acov(x, K):
    n = x.shape[0]
    m = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(x, m)
    return np.fft.irfft(f * np.conj(f), m)[:K + 1] / (n - np.arange(K + 1))


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def tica_legs(a, A, dev, want):
    NF, lag = 25, 1000
    for n in (100000, 1000000):
        if not (want("moments") or (n == 1000000 and want("project"))):
            continue
        ang = angles(n, NF, dev)
        D, m = 2 * NF, n - lag
        if want("moments"):
            ws = torch.empty(A.lagged_moments_workspace_bytes(n, NF, lag), dtype=torch.uint8, device=dev)
            sx, sy = (torch.empty(D, dtype=torch.float64, device=dev) for _ in range(2))
            cxx, cyy, cxy = (torch.empty(D, D, dtype=torch.float64, device=dev) for _ in range(3))
            best, med = timed_ms(lambda: A.lagged_moments_into(ang, lag, sx, sy, cxx, cyy, cxy, ws), a.reps)

            def on_host():
                x = host_features(ang)
                X, Y = x[:m], x[lag:]
                return X.sum(0), Y.sum(0), X.T @ X, Y.T @ Y, X.T @ Y
            ref = on_host()
            err = max(float(np.abs(g.cpu().numpy() - w).max()) / m for g, w in zip((sx, sy, cxx, cyy, cxy), ref))
            rate = 3.0 * D * D * m / (best * 1e-3)
            print(json.dumps({"leg": "moments", "n": n, "NF": NF, "lag": lag, "ms_best": best, "ms_median": med,
                              "workspace_MB": ws.numel() / 1e6, "fma_per_s": rate, "share_of_fp32_vector_peak": rate / FMA_PEAK,
                              "feature_read_GB_per_s": 2 * n * D * 4 / best / 1e6, "max_abs_err_over_m": err,
                              "numpy_ms": host_ms(on_host)}))
        if want("project") and n == 1000000:
            g = torch.Generator().manual_seed(2)
            mean = (0.3 * torch.randn(D, generator=g)).to(dev)
            for d in (2, 10):
                W = torch.randn(D, d, generator=g).to(dev)
                out = torch.empty(n, d, device=dev)
                best, med = timed_ms(lambda: A.project_into(ang, mean, W, out), a.reps)
                on_host = lambda: (host_features(ang) - mean.double().cpu().numpy()) @ W.double().cpu().numpy()   # noqa: E731
                err = float(np.abs(out.cpu().numpy() - on_host()).max())
                print(json.dumps({"leg": "project", "n": n, "NF": NF, "d": d, "ms_best": best, "ms_median": med,
                                  "GB_per_s": (ang.numel() + out.numel()) * 4 / best / 1e6, "max_abs_err": err,
                                  "numpy_ms": host_ms(on_host)}))
    if want("series"):
        for size in [s for s in SIZES if a.size in ("both", s)]:
            n, K, _ = SIZES[size]
            x = (3.0 * angles(n, 1, dev) + 0.5).contiguous()
            ws = torch.empty(A.series_acov_workspace_bytes(n, 1, K), dtype=torch.uint8, device=dev)
            acov = torch.empty(1, K + 1, dtype=torch.float64, device=dev)
            mean = torch.empty(1, dtype=torch.float64, device=dev)
            best, med = timed_ms(lambda: A.series_acov_into(x, K, acov, mean, ws), a.reps)
            on_host = lambda: host_acov(x[:, 0].double().cpu().numpy(), K)   # noqa: E731
            err = float(np.abs(acov[0].cpu().numpy() - on_host()).max())
            rate = macs(n, K, 1) / 2 / (best * 1e-3)
            print(json.dumps({"leg": "series", "size": size, "n": n, "K": K, "NS": 1, "ms_best": best, "ms_median": med,
                              "fma_per_s": rate, "share_of_fp32_vector_peak": rate / FMA_PEAK, "max_abs_err": err,
                              "numpy_ms": host_ms(on_host)}))
    if want("tica"):
        aat = np.array([3, 10, 1, 8])
        g = torch.Generator(device=dev).manual_seed(3)
        traj = torch.randn(100000, 4, 14, 3, generator=g, device=dev) * 3
        ref = torch.randn(1000000, 4, 14, 3, generator=g, device=dev) * 3
        plain_best, plain_med = timed_ms(lambda: A.analyze(traj, ref, aat), max(a.reps // 2, 1))
        best, med = timed_ms(lambda: A.analyze(traj, ref, aat, tica=True), max(a.reps // 2, 1))
        a_traj, a_ref = A.featurize(traj, aat), A.featurize(ref, aat)

        def on_host():
            xr, xt = host_features(a_ref), host_features(a_traj)
            mm = xr.shape[0] - A.TICA_LAG
            X, Y = xr[:mm], xr[A.TICA_LAG:]
            model = A.tica_solve(mm, X.sum(0), Y.sum(0), X.T @ X, Y.T @ Y, X.T @ Y, lag=A.TICA_LAG)
            yr, yt = ((x - model.mean) @ model.W[:, :max(model.dim, 2)] for x in (xr, xt))
            lo, hi = np.minimum(yr[:, :2].min(0), yt[:, :2].min(0)), np.maximum(yr[:, :2].max(0), yt[:, :2].max(0))
            rng = ((lo[0], hi[0]), (lo[1], hi[1]))
            j1 = A.jsd(*(np.histogram(y[:, 0], range=rng[0], bins=100)[0] for y in (yr, yt)))
            j2 = A.jsd(*(np.histogram2d(y[:, 0], y[:, 1], range=rng, bins=50)[0] for y in (yr, yt)))
            return j1, j2, host_acov(yr[:, 0], A.MD_NLAG), host_acov(yt[:, 0], A.NLAG)
        print(json.dumps({"leg": "tica", "frames": 100000, "md_frames": 1000000, "NF": a_ref.shape[1], "tica_lag": A.TICA_LAG,
                          "analyze_ms_best": plain_best, "analyze_ms_median": plain_med, "analyze_tica_ms_best": best,
                          "analyze_tica_ms_median": med, "tica_part_ms": best - plain_best, "numpy_ms": host_ms(on_host)}))


def wall_ms(fn, reps):
    """Best and median wall time of `reps` calls, the device idle before and after each."""
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms))


def host_lloyd_step(x, c):
    """One Lloyd step in NumPy fp64 (distances in blocks of 1e4 points)."""
    x, c = x.astype(np.float64), c.astype(np.float64)
    arg = np.empty(len(x), np.int64)
    cost = 0.0
    for i in range(0, len(x), 10000):
        D = ((x[i:i + 10000, None, :] - c[None]) ** 2).sum(-1)
        arg[i:i + 10000] = D.argmin(1)
        cost += D.min(1).sum()
    sums = np.zeros_like(c)
    np.add.at(sums, arg, x)
    counts = np.bincount(arg, minlength=len(c))
    return np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], c), cost


def msm_legs(a, A, dev, want):
    n, d, k = 1000000, 10, 100
    if any(want(leg) for leg in ("kmeans_pp", "kmeans_step", "kmeans_fit", "count_matrix")):
        x = angles(n, d, dev)
        u = np.random.default_rng(A.KMEANS_SEED).random(k)
        chosen = A.kmeans_pp(x, k, u)
        centers0 = x.index_select(0, chosen).contiguous()
    if want("kmeans_pp"):
        ch = torch.zeros(k, dtype=torch.int64, device=dev)
        mind2 = torch.empty(n, device=dev)
        ws = torch.empty(A.kmeans_pp_workspace_bytes(n, d, k), dtype=torch.uint8, device=dev)
        best, med = timed_ms(lambda: A.kmeans_pp_into(x, k, u, 0, k, ch, mind2, ws), a.reps)
        print(json.dumps({"leg": "kmeans_pp", "n": n, "d": d, "k": k, "ms_best": best, "ms_median": med, "ms_per_round": best / k,
                          "distinct": int(ch.unique().numel())}))
    if want("kmeans_step"):
        centers = centers0.clone()
        assign = torch.empty(n, dtype=torch.int32, device=dev)
        sums = torch.empty(k, d, dtype=torch.float64, device=dev)
        counts = torch.empty(k, dtype=torch.int64, device=dev)
        cost, state = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        ws = torch.empty(A.kmeans_step_workspace_bytes(n, d, k), dtype=torch.uint8, device=dev)

        def step():
            centers.copy_(centers0)
            state.zero_()
            A.kmeans_step_into(x, centers, assign, sums, counts, cost, state, 0.0, ws)
        best, med = timed_ms(step, a.reps)
        xs, cs = x[:100000].cpu().numpy(), centers0.cpu().numpy()
        print(json.dumps({"leg": "kmeans_step", "n": n, "d": d, "k": k, "ms_best": best, "ms_median": med,
                          "workspace_MB": ws.numel() / 1e6, "distance_fma_per_s": float(n) * k * d / (best * 1e-3),
                          "share_of_fp32_vector_peak": float(n) * k * d / (best * 1e-3) / FMA_PEAK,
                          "numpy_step_ms_1e5": host_ms(lambda: host_lloyd_step(xs, cs))}))
    if want("kmeans_fit"):
        fit = A.kmeans_fit(x, k)
        best, med = wall_ms(lambda: A.kmeans_fit(x, k), max(a.reps // 2, 1))
        print(json.dumps({"leg": "kmeans_fit", "n": n, "d": d, "k": k, "max_iter": A.KMEANS_MAX_ITER, "steps": fit["steps"],
                          "wall_ms_best": best, "wall_ms_median": med}))
    if want("count_matrix"):
        for kk in (100, 256):
            cen = x[torch.randperm(n, generator=torch.Generator().manual_seed(4))[:kk].to(dev)].contiguous()
            dtraj = A.kmeans_assign(x, cen)
            cm = torch.empty(kk, kk, dtype=torch.int64, device=dev)
            dr = torch.empty(1, dtype=torch.int64, device=dev)
            best, med = timed_ms(lambda: A.count_matrix_into(dtraj, 1000, kk, cm, dr), a.reps * 4)
            abest, _ = timed_ms(lambda: A.kmeans_assign(x, cen), a.reps)
            print(json.dumps({"leg": "count_matrix", "n": n, "lag": 1000, "k": kk, "ms_best": best, "ms_median": med,
                              "nonzero_cells": int((cm > 0).sum()), "assign_ms_best": abest}))
    if want("msm"):
        from mdgen_amd import msm as M
        aat = np.array([3, 10, 1, 8])
        g = torch.Generator(device=dev).manual_seed(3)
        traj = torch.randn(100000, 4, 14, 3, generator=g, device=dev) * 3
        ref = torch.randn(1000000, 4, 14, 3, generator=g, device=dev) * 3
        reps = max(a.reps // 2, 1)
        tica_best, tica_med = wall_ms(lambda: A.analyze(traj, ref, aat, tica=True), reps)
        best, med = wall_ms(lambda: A.analyze(traj, ref, aat, msm=True), reps)
        out = A.analyze(traj, ref, aat, msm=True)      # (frames drawn independently: every microstate reaches every other)

        def on_host():
            C = out["msm"]["count_matrix"]
            m = M.estimate_msm(C, A.MD_MSM_LAG)
            M.pcca(m["transition_matrix"], m["pi"], A.MSM_STATES)
        print(json.dumps({"leg": "msm", "frames": 100000, "md_frames": 1000000, "dim": out["kmeans"]["dim"], "k": A.KMEANS_K,
                          "kmeans_steps": out["kmeans"]["steps"], "analyze_tica_wall_ms_best": tica_best,
                          "analyze_tica_wall_ms_median": tica_med, "analyze_msm_wall_ms_best": best, "analyze_msm_wall_ms_median": med,
                          "msm_part_ms": best - tica_best, "host_ms": host_ms(on_host)}))


def tps_legs(a, A, dev, want):
    if not want("tps"):
        return
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import tps_ref as R
    from mdgen_amd import analyze_peptide_tps as tps
    from mdgen_amd import msm as M
    from mdgen_amd.tps_inference import build_metadata
    k = 10
    Ta, Tb, phi = R.chain(k, 1, 0.2), R.chain(k, 2, 0.1), np.arange(k, dtype=np.int32)[::-1].copy()
    start, end = 0, k - 1
    for n, N in ((1000, 11), (1000000, 101)):
        Ba, Bb = M.bridge_table(Ta, end, N), M.bridge_table(Tb, int(phi[end]), N)
        dTa, dBa, dTb, dBb = (torch.from_numpy(x).to(dev) for x in (Ta, Ba, Tb, Bb))
        paths = torch.empty(n, N, dtype=torch.int32, device=dev)
        prob = torch.empty(n, dtype=torch.float64, device=dev)
        reps = a.reps * 4 if n == 1000 else a.reps
        best, med = timed_ms(lambda: A.tp_sample_into(dTa, dBa, start, end, 137, 0, paths, Tb=dTb, Bb=dBb, phi=phi, prob=prob), reps)
        wbest, wmed = wall_ms(lambda: A.tp_sample(Ta, start, end, N, n, 137, 0, score=(Tb, phi)), reps)

        def on_host():
            p = R.sample(Ta, M.bridge_table(Ta, end, N), start, end, n, 137, 0)
            return p, M.tp_likelihood(phi[p], Tb).prod(-1)
        t0 = time.perf_counter()
        hp, hq = on_host()
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(hp, paths.cpu().numpy()) and np.allclose(hq, prob.cpu().numpy(), rtol=1e-12, atol=0))
        print(json.dumps({"leg": "tps", "what": "sampler", "n_samples": n, "N": N, "k": k, "kernel_ms_best": best,
                          "kernel_ms_median": med, "steps_per_s": float(n) * (N - 2) / (best * 1e-3), "tp_sample_wall_ms_best": wbest,
                          "tp_sample_wall_ms_median": wmed, "numpy_ms": numpy_ms, "equal_to_numpy": same}))
    # one peptide of analyze_peptide_tps at the reference's size (frames drawn independently: every microstate reaches every other)
    aat = np.array([3, 10, 1, 8])
    g = torch.Generator(device=dev).manual_seed(3)
    md = torch.randn(1000000, 4, 14, 3, generator=g, device=dev) * 3
    t0 = time.perf_counter()
    pkl = build_metadata(md, aat, device=dev)
    torch.cuda.synchronize()
    meta_ms = (time.perf_counter() - t0) * 1e3
    del md
    s_state, e_state, si, ei = M.tps_endpoints(pkl["cmsm"], pkl["pcca"]["metastable_assignments"], pkl["ref_kmeans"], 1000, 137, 0)
    records = [{"start_state": s_state, "end_state": e_state}] * 1000
    gen = (torch.randn(1000, 100, 4, 14, 3, generator=g, device=dev) * 3).cpu().numpy()
    rep = (torch.randn(1000000, 4, 14, 3, generator=g, device=dev) * 3).cpu().numpy()
    kept = gen[:, tps.strided_frames(100, 10)]
    best, med = wall_ms(lambda: tps.analyze_tps("bench", pkl, records, kept, aat, rep, device=dev), max(a.reps // 2, 1))
    nbest, _ = wall_ms(lambda: tps.analyze_tps("bench", pkl, records, kept, aat, None, device=dev), max(a.reps // 2, 1))
    print(json.dumps({"leg": "tps", "what": "analyze_peptide_tps", "paths": 1000, "frames": 100, "kept": kept.shape[1],
                      "replica_frames": 1000000, "rep_lens": len(tps.REP_LENS), "n_samples": 1000, "wall_ms_best": best,
                      "wall_ms_median": med, "without_replica_wall_ms_best": nbest, "metadata_wall_ms": meta_ms}))


def ensemble_legs(a, dev):
    from mdgen_amd import ensemble as E
    L, T, F = 256, 250, 30003
    g = torch.Generator(device=dev).manual_seed(7)
    aat = np.random.default_rng(7).integers(0, 20, size=L)
    w, ex = E.fit_weights(aat, "heavy")
    mask = torch.from_numpy(ex.reshape(L, 14, 1).astype(np.float32)).to(dev)
    idx = torch.arange(L, device=dev, dtype=torch.float32)
    ca = torch.stack([2.3 * torch.cos(idx * 1.75), 2.3 * torch.sin(idx * 1.75), 1.5 * idx], -1)
    ca = ca + torch.cumsum(torch.randn(L, 3, generator=g, device=dev) * 2.0, 0)        # a wandering chain: ~30 A across
    base = ca[:, None, :] + torch.randn(L, 14, 3, generator=g, device=dev) * 1.8
    md = (base + torch.randn(F, L, 1, 3, generator=g, device=dev) * 1.0 + torch.randn(F, L, 14, 3, generator=g, device=dev) * 0.3) * mask
    tr = (base + torch.randn(T, L, 1, 3, generator=g, device=dev) * 0.8 + torch.randn(T, L, 14, 3, generator=g, device=dev) * 0.3) * mask
    if a.leg == "sasa":
        return sasa_records(a, dev, tr, md, aat)
    x = md.reshape(F, L * 14, 3)
    wd, exd = torch.from_numpy(w).to(dev), torch.from_numpy(ex).to(dev)
    out = torch.empty_like(x)
    best, med = timed_ms(lambda: E.superpose_into(x, x[0], wd, exd, out), a.reps)
    print(json.dumps({"leg": "ensemble", "what": "superpose", "F": F, "A": L * 14, "ms_best": best, "ms_median": med,
                      "GB_per_s": 2 * x.numel() * 4 / best / 1e6}))
    mean, cov = torch.empty(L * 14, 3, dtype=torch.float64, device=dev), torch.empty(L * 14, 3, 3, dtype=torch.float64, device=dev)
    ws = torch.empty(E.moments_workspace_bytes(F, L * 14), dtype=torch.uint8, device=dev)
    best, med = timed_ms(lambda: E.moments_into(out, mean, cov, ws), a.reps)
    print(json.dumps({"leg": "ensemble", "what": "moments", "F": F, "A": L * 14, "ms_best": best, "ms_median": med,
                      "GB_per_s": x.numel() * 4 / best / 1e6}))
    del out
    small = torch.randn(1000000, 56, 3, generator=g, device=dev) * 5
    w56, o56 = torch.ones(56, device=dev), torch.empty(1000000, 56, 3, device=dev)
    best, med = timed_ms(lambda: E.superpose_into(small, small[0], w56, None, o56), a.reps)
    print(json.dumps({"leg": "ensemble", "what": "superpose", "F": 1000000, "A": 56, "ms_best": best, "ms_median": med,
                      "GB_per_s": 2 * small.numel() * 4 / best / 1e6}))
    del small, o56
    ca_md, ca_tr = md[:, :, 1].contiguous(), tr[:, :, 1].contiguous()
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    c2 = float(E.cutoff2_f32(8.0))

    def cdist_sums(xa, xb, mode):
        A_ = xa.shape[1]
        fa, fb = xa.reshape(len(xa), -1), xb.reshape(len(xb), -1)
        s0 = torch.zeros((), dtype=torch.float64, device=dev)
        s1 = torch.zeros((), dtype=torch.float64, device=dev)
        for i in range(0, len(fa), 2048):
            d = torch.cdist(fa[i:i + 2048], fb, compute_mode=mode)
            s0 += (d.double() / np.sqrt(A_)).sum()
            s1 += (d.double() ** 2 / A_).sum()
        return torch.stack([s0, s1])
    wide = (ca_md.repeat(1, 4, 1) + torch.randn(F, 1024, 3, generator=g, device=dev) * 0.5).contiguous()
    for name, xa, xb in (("sampled x md", ca_tr, ca_md), ("md x md", ca_md, ca_md), ("md x md, A = 1024", wide, wide)):
        Fa, Fb, A_ = len(xa), len(xb), xa.shape[1]
        ws = torch.empty(E.pairwise_workspace_bytes(Fa, Fb, A_), dtype=torch.uint8, device=dev)
        best, med = timed_ms(lambda: E.pairwise_d2_into(xa, xb, None, sums, ws), a.reps)
        got = sums.cpu().numpy()
        rate = float(Fa) * Fb * 3 * A_ / (best * 1e-3)
        rec = {"leg": "ensemble", "what": "pairwise_d2", "shape": name, "Fa": Fa, "Fb": Fb, "A": A_, "ms_best": best, "ms_median": med,
               "fma_per_s": rate, "share_of_fp32_vector_peak": rate / FMA_PEAK}
        for key, mode in (("torch_cdist_mm_ms", "use_mm_for_euclid_dist"), ("torch_cdist_direct_ms", "donot_use_mm_for_euclid_dist")):
            tb, _ = timed_ms(lambda: cdist_sums(xa, xb, mode), max(a.reps // 2, 1))
            ref = cdist_sums(xa, xb, mode).cpu().numpy()
            rec[key] = tb
            rec[key.replace("_ms", "_rel_diff")] = float(np.abs(ref - got).max() / np.abs(got).max())
        print(json.dumps(rec))
    del wide
    counts = torch.empty(L, L, dtype=torch.int32, device=dev)

    def torch_contacts(ca_):
        acc = torch.zeros(L, L, dtype=torch.int64, device=dev)
        for i in range(0, len(ca_), 512):
            c = ca_[i:i + 512]
            d = c[:, :, None, :] - c[:, None, :, :]
            acc += ((d * d).sum(-1) < c2).sum(0)
        return acc
    for name, ca_ in (("sampled", ca_tr), ("md", ca_md)):
        best, med = timed_ms(lambda: E.contact_counts_into(ca_, 8.0, counts), a.reps)
        tb, _ = timed_ms(lambda: torch_contacts(ca_), max(a.reps // 2, 1))
        diff = int((torch_contacts(ca_) - counts).abs().max())
        print(json.dumps({"leg": "ensemble", "what": "contact_counts", "shape": name, "F": len(ca_), "N": L, "ms_best": best,
                          "ms_median": med, "torch_chunked_ms": tb, "max_count_diff_to_torch": diff,
                          "contact_share": float(counts.double().mean() / len(ca_))}))
    for pca in (False, True):
        best, med = wall_ms(lambda: E.analyze_ensemble(tr, md, aat, pca=pca), max(a.reps // 2, 1))
        print(json.dumps({"leg": "ensemble", "what": "analyze_ensemble", "pca": pca, "T": T, "F": F, "L": L, "wall_ms_best": best,
                          "wall_ms_median": med}))
    sasa_records(a, dev, tr, md, aat, with_plain=False)


def torch_sasa_counts(x, rad, pts, probe, atoms_at_a_time=16):
    """The counts of `mdgen_ens_sasa_counts` as plain torch expressions, frame by frame and 16 atoms at a time."""
    dev = x.device
    live = torch.from_numpy(np.flatnonzero(rad != 0)).to(dev)
    R = torch.from_numpy((rad[rad != 0] + np.float32(probe)).astype(np.float32)).to(dev)
    R2 = R * R
    u = torch.from_numpy(pts).to(dev)
    counts = torch.zeros(x.shape[0], x.shape[1], dtype=torch.int32, device=dev)
    n = len(live)
    for f in range(x.shape[0]):
        c = x[f, live]
        for i0 in range(0, n, atoms_at_a_time):
            k = min(atoms_at_a_time, n - i0)
            q = c[i0:i0 + k, None, :] + R[i0:i0 + k, None, None] * u[None]                      # [k, P, 3]
            d = q[:, :, None, 0] - c[None, None, :, 0]
            d2 = d * d
            for ax in (1, 2):
                d = q[:, :, None, ax] - c[None, None, :, ax]
                d2 += d * d
            hit = d2 < R2[None, None, :]
            own = torch.arange(k, device=dev)
            hit[own, :, i0 + own] = False
            counts[f, live[i0:i0 + k]] = (~hit.any(-1)).sum(-1).to(torch.int32)
    return counts


def sasa_records(a, dev, tr, md, aat, with_plain=True):
    from mdgen_amd import ensemble as E
    L, P, probe = len(aat), 960, 2.8
    rad, pts = E.atom_radii(aat), E.sphere_points(P)
    ws = torch.empty(E.sasa_workspace_bytes(L * 14, P), dtype=torch.uint8, device=dev)
    for name, coords in (("sampled", tr), ("md", md)):
        x = coords.reshape(len(coords), L * 14, 3)
        counts = torch.empty(len(x), L * 14, dtype=torch.int32, device=dev)
        best, med = timed_ms(lambda: E.sasa_counts_into(x, rad, pts, probe, counts, ws), a.reps)
        nt = min(a.sasa_torch_frames, len(x))
        tb, _ = timed_ms(lambda: torch_sasa_counts(x[:nt], rad, pts, probe), 1)
        diff = int((torch_sasa_counts(x[:nt], rad, pts, probe) != counts[:nt]).sum())
        live = int((rad != 0).sum())
        print(json.dumps({"leg": "ensemble", "what": "sasa_counts", "shape": name, "F": len(x), "A": L * 14, "existing_atoms": live,
                          "P": P, "probe": probe, "ms_best": best, "ms_median": med, "ms_per_frame": best / len(x),
                          "torch_frames": nt, "torch_ms": tb, "torch_ms_per_frame": tb / nt,
                          "entries_differing_from_torch": diff, "entries_compared": nt * L * 14,
                          "exposed_share": float(counts.double().sum() / (len(x) * live * P))}))
    for sasa in ((False, True) if with_plain else (True,)):
        best, med = wall_ms(lambda: E.analyze_ensemble(tr, md, aat, pca=False, sasa=sasa), max(a.reps // 2, 1))
        print(json.dumps({"leg": "ensemble", "what": "analyze_ensemble", "pca": False, "sasa": sasa, "T": len(tr), "F": len(md), "L": L,
                          "wall_ms_best": best, "wall_ms_median": med}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="all", choices=["all", "dihedrals", "histograms", "acov", "fft", "numpy", "moments", "project",
                                                     "series", "tica", "kmeans_pp", "kmeans_step", "kmeans_fit", "count_matrix",
                                                     "msm", "tps", "ensemble", "sasa"])
    ap.add_argument("--size", default="both", choices=["sampler", "md", "both"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sasa_torch_frames", type=int, default=4, help="ensemble / sasa legs: frames of the torch restatement of the counts")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("analysis_bench needs the GPU: there is nothing to time without one")
    from mdgen_amd import analysis as A
    dev = torch.device("cuda")
    if a.leg in ("ensemble", "sasa"):
        return ensemble_legs(a, dev)
    want = lambda leg: a.leg in ("all", leg)   # noqa: E731
    sizes = [s for s in SIZES if a.size in ("both", s)]
    F = 100000
    if want("dihedrals") or want("histograms"):
        for seq in ([3, 10, 1, 8], [3, 10, 1, 8, 17, 11, 6, 13]):
            aat = np.array(seq)
            labels, quad = A.torsion_features(aat)
            atom14 = (torch.randn(F, len(aat), 14, 3, generator=torch.Generator().manual_seed(1)) * 3).to(dev)
            ang = torch.empty(F, len(quad), device=dev)
            if want("dihedrals"):
                best, med = timed_ms(lambda: A.dihedrals_into(atom14, quad, ang), a.reps * 4)
                print(json.dumps({"leg": "dihedrals", "F": F, "L": len(aat), "NF": len(quad), "ms_best": best, "ms_median": med,
                                  "GB_per_s": (atom14.numel() + ang.numel()) * 4 / best / 1e6}))
            if want("histograms"):
                A.dihedrals_into(atom14, quad, ang)
                pairs = np.array(A.DEFAULT_PAIRS, np.int32)
                e1, e2 = (torch.from_numpy(A.hist_edges(b)).to(dev) for b in (A.BINS_1D, A.BINS_2D))
                h1 = torch.empty(len(quad), A.BINS_1D, dtype=torch.int64, device=dev)
                h2 = torch.empty(2, A.BINS_2D, A.BINS_2D, dtype=torch.int64, device=dev)
                dr = torch.empty(len(quad) + 2, dtype=torch.int64, device=dev)
                best, med = timed_ms(lambda: A.histograms_into(ang, pairs, A.BINS_1D, e1, A.BINS_2D, e2, h1, h2, dr), a.reps * 4)
                print(json.dumps({"leg": "histograms", "F": F, "NF": len(quad), "P": 2, "ms_best": best, "ms_median": med}))
    for size in sizes:
        n, K, NF = SIZES[size]
        ang = angles(n, NF, dev)
        if want("acov"):
            ws = torch.empty(A.acov_workspace_bytes(n, NF, K), dtype=torch.uint8, device=dev)
            acov = torch.empty(NF, K + 1, dtype=torch.float64, device=dev)
            ms_, mc_ = torch.empty(NF, dtype=torch.float64, device=dev), torch.empty(NF, dtype=torch.float64, device=dev)
            best, med = timed_ms(lambda: A.acov_into(ang, K, acov, ms_, mc_, ws), a.reps)
            rate = macs(n, K, NF) / (best * 1e-3)
            print(json.dumps({"leg": "acov", "size": size, "n": n, "K": K, "NF": NF, "ms_best": best, "ms_median": med,
                              "workspace_MB": ws.numel() / 1e6, "fma_per_s": rate, "share_of_fp32_vector_peak": rate / FMA_PEAK}))
        if want("fft"):
            m = 1 << int(np.ceil(np.log2(2 * n)))

            def via_fft():
                out = 0
                for x in (torch.sin(ang), torch.cos(ang)):
                    f = torch.fft.rfft(x.t().contiguous(), m)
                    out = out + torch.fft.irfft(f * f.conj(), m)[:, :K + 1]
                return out / (n - torch.arange(K + 1, device=dev))
            best, med = timed_ms(via_fft, a.reps)
            print(json.dumps({"leg": "fft", "size": size, "n": n, "K": K, "NF": NF, "fft_points": m, "dtype": "float32",
                              "ms_best": best, "ms_median": med}))
            if want("acov"):   # what the fp32 FFT costs in accuracy, beside the kernel, against the fp64 FFT on the host (one feature)
                a64 = ang[:, :1].double().cpu().numpy()
                ref = np.zeros(K + 1)
                for x in (np.sin(a64[:, 0]), np.cos(a64[:, 0])):
                    f = np.fft.rfft(x, m)
                    ref += np.fft.irfft(f * np.conj(f), m)[:K + 1]
                ref /= n - np.arange(K + 1)
                print(json.dumps({"leg": "accuracy", "size": size, "max_abs_err_kernel": float(np.abs(acov[0].cpu().numpy() - ref).max()),
                                  "max_abs_err_torch_fft_fp32": float(np.abs(via_fft()[0].double().cpu().numpy() - ref).max())}))
        if want("numpy") and size == "sampler":
            host = ang.double().cpu().numpy()
            m = 1 << int(np.ceil(np.log2(2 * n)))
            t0 = time.perf_counter()
            out = np.zeros((K + 1, NF))
            for x in (np.sin(host), np.cos(host)):
                f = np.fft.rfft(x, m, axis=0)
                out += np.fft.irfft(f * np.conj(f), m, axis=0)[:K + 1]
            dt = time.perf_counter() - t0
            print(json.dumps({"leg": "numpy", "size": size, "n": n, "K": K, "NF": NF, "dtype": "float64", "ms": dt * 1e3}))
    tica_legs(a, A, dev, want)
    msm_legs(a, A, dev, want)
    tps_legs(a, A, dev, want)


if __name__ == "__main__":
    main()
