"""csrc/k_msm.hip and the chain around it on the GPU against tests/msm_ref.py (gates: its docstring).

Every output buffer is pre-filled with a sentinel and has a guard region of the sentinel behind it; the guards must be intact, no
sentinel may be left where an output belongs, and a second call gives the same bits.  Count matrices are compared with np.add.at,
exactly."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref as R  # noqa: E402
import msm_ref as K  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
SENT_F = -7777.0
SENT_I = -77777


def _cuda():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _guarded(n, dtype, sentinel):
    buf = torch.full((n + GUARD,), sentinel, dtype=dtype, device=_cuda())
    return buf, buf[:n]


def _guard_ok(buf, n, sentinel):
    assert (buf[n:] == sentinel).all().item(), "guard overwritten"


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(_cuda())   # (a copy: the cases are read-only)


# ---- assignment ------------------------------------------------------------------------------------------------------
def run_assign(x, c, with_dist2=True):
    from mdgen_amd.analysis import kmeans_assign_into
    n = len(x)
    ba, assign = _guarded(n, torch.int32, SENT_I)
    bd, d2 = _guarded(n, torch.float32, SENT_F)
    kmeans_assign_into(_dev(x), _dev(c), assign, d2 if with_dist2 else None)
    torch.cuda.synchronize()
    _guard_ok(ba, n, SENT_I)
    if with_dist2:
        _guard_ok(bd, n, SENT_F)
    else:
        assert (bd == SENT_F).all().item()
    a, dd = assign.cpu().numpy(), d2.cpu().numpy()
    assert not (a == SENT_I).any() and not (with_dist2 and (dd == SENT_F).any()), "an output was not written"
    return a, dd


def check_assignment(x, c, a, d2=None):
    """The device's assignment `a` (and distances) of x to the centres c against fp64; the share of undecided points."""
    n, k = len(x), len(c)
    arg, dmin, decided, g = K.assign(x, c)
    assert a.min() >= 0 and a.max() < k
    assert np.array_equal(a[decided], arg[decided]), "a decided point is not with its nearest centre"
    D = K.dist2(x, c)
    own = D[np.arange(n), a]
    assert (own - dmin <= 2.0 * g).all()                  # an undecided point is with one of its near-equal centres
    if d2 is not None:
        err = np.abs(d2.astype(np.float64) - own)
        print(f"  dist2: worst error / gate {np.max(err / g):.3f}")
        assert (err <= g).all()
    share = float((~decided).mean())
    print(f"  undecided {int((~decided).sum())} of {n} ({share:.4%})")
    assert share <= K.UNDECIDED_CAP
    return decided


@pytest.mark.parametrize("n,d,k,seed", K.ASSIGN_CASES)
def test_kmeans_assign(n, d, k, seed):
    x, c = K.inputs(n, d, k, seed)
    a, d2 = run_assign(x, c)
    check_assignment(x, c, a, d2)
    a2, d22 = run_assign(x, c)
    assert np.array_equal(a, a2) and np.array_equal(d2, d22), "a second call gave other bits"
    assert np.array_equal(run_assign(x, c, with_dist2=False)[0], a)
    if 1 < k < 256:                                       # equal centres: the tie goes to the lowest index
        dup = np.concatenate([c[-1:], c])
        assert (run_assign(x, dup)[0] != k).all()


def test_kmeans_assign_refusal_leaves_the_outputs_alone():
    from mdgen_amd._lib import MdgenError, launch, lib, ptr
    dev = _cuda()
    buf, out = _guarded(64, torch.int32, SENT_I)
    x, c = torch.zeros(8, 2, device=dev), torch.zeros(3, 2, device=dev)
    for d, k in ((0, 3), (129, 3), (2, 0), (2, 257)):
        with pytest.raises(MdgenError, match="must be in 1 .."):
            launch(lib.mdgen_traj_kmeans_assign, x, 8, d, k, ptr(x), ptr(c), ptr(out), None)
    torch.cuda.synchronize()
    assert (buf == SENT_I).all().item()


# ---- one Lloyd step --------------------------------------------------------------------------------------------------
class Step:
    """Guarded buffers of `kmeans_step_into` for x (n, d) and centres c (k, d)."""

    def __init__(self, x, c, state=(0, 0), cost=(0.0, 0.0)):
        from mdgen_amd.analysis import kmeans_step_workspace_bytes
        self.n, self.d, self.k = len(x), x.shape[1], len(c)
        n, d, k = self.n, self.d, self.k
        self.x = _dev(x)
        self.bufs = {"centers": _guarded(k * d, torch.float32, SENT_F), "assign": _guarded(n, torch.int32, SENT_I),
                     "sums": _guarded(k * d, torch.float64, SENT_F), "counts": _guarded(k, torch.int64, SENT_I),
                     "cost": _guarded(2, torch.float64, SENT_F), "state": _guarded(2, torch.int32, SENT_I)}
        self.bufs["centers"][1].copy_(_dev(c).reshape(-1))
        self.bufs["cost"][1].copy_(torch.tensor(cost, dtype=torch.float64))
        self.bufs["state"][1].copy_(torch.tensor(state, dtype=torch.int32))
        self.ws = torch.full((kmeans_step_workspace_bytes(n, d, k) + GUARD,), 0x5A, dtype=torch.uint8, device=_cuda())

    def run(self, tol=1e-5):
        from mdgen_amd.analysis import kmeans_step_into
        v = {key: b[1] for key, b in self.bufs.items()}
        kmeans_step_into(self.x, v["centers"].view(self.k, self.d), v["assign"], v["sums"], v["counts"], v["cost"], v["state"], tol,
                         self.ws[:-GUARD])
        torch.cuda.synchronize()
        for key, (b, view) in self.bufs.items():
            _guard_ok(b, view.numel(), SENT_I if b.dtype in (torch.int32, torch.int64) else SENT_F)
        assert (self.ws[-GUARD:] == 0x5A).all().item(), "workspace guard overwritten"
        out = {key: view.cpu().numpy().copy() for key, (b, view) in self.bufs.items()}
        out["centers"], out["sums"] = out["centers"].reshape(self.k, self.d), out["sums"].reshape(self.k, self.d)
        return out


def check_step(x, c_old, got, prev_cost, steps_before):
    """One executed step's outputs against fp64 recomputed from the device's own assignment and distances."""
    k = len(c_old)
    a, d2 = run_assign(x, c_old)
    assert np.array_equal(got["assign"], a), "the step's assignment is not mdgen_traj_kmeans_assign's"
    sums, mags, counts = K.cluster_sums(x, a, k)
    assert np.array_equal(got["counts"], counts)
    assert (np.abs(got["sums"] - sums) <= K.SUM_RTOL * mags).all()
    cost = d2.astype(np.float64).sum()
    assert abs(got["cost"][0] - cost) <= K.SUM_RTOL * cost and got["cost"][1] == prev_cost
    assert got["state"][1] == steps_before + 1
    live = counts > 0
    want = np.array(c_old, np.float32)
    want[live] = (got["sums"][live] / got["counts"][live, None]).astype(np.float32)       # of the device's own sums: bit for bit
    assert np.array_equal(got["centers"], want)
    return a


@pytest.mark.parametrize("n,d,k,seed", K.ASSIGN_CASES)
def test_kmeans_step(n, d, k, seed):
    x, c = K.inputs(n, d, k, seed)
    s = Step(x, c)
    one = s.run(tol=0.0)
    a = check_step(x, c, one, 0.0, 0)
    check_assignment(x, c, a)
    assert one["state"][0] == 0                                       # the first step never sets the flag
    again = Step(x, c).run(tol=0.0)
    assert all(np.array_equal(one[key], again[key]) for key in one), "a second call gave other bits"
    two = s.run(tol=0.0)                                              # the second step, from the first's centres
    check_step(x, one["centers"], two, one["cost"][0], 1)
    assert two["cost"][0] <= one["cost"][0] * (1 + 1e-6)
    assert two["state"][0] == (1 if two["cost"][0] == one["cost"][0] else 0)      # tol 0: done only when the cost repeats


def test_kmeans_step_empty_cluster_keeps_its_centre():
    x, c = K.inputs(257, 5, 3, 23)
    c = np.concatenate([c[:1], np.full((1, 5), 1e3, np.float32), c[1:]])          # centre 1 is far from every point
    got = Step(x, c).run()
    check_step(x, c, got, 0.0, 0)
    assert got["counts"][1] == 0 and (got["sums"][1] == 0).all() and np.array_equal(got["centers"][1], c[1])
    assert got["counts"].sum() == 257


def test_kmeans_step_done_flag():
    x, c = K.inputs(4099, 2, 8, 11)
    s = Step(x, c, state=(1, 5), cost=(3.0, 4.0))                    # the flag set: nothing may change, sentinels included
    got = s.run()
    assert np.array_equal(got["centers"], c) and (got["assign"] == SENT_I).all() and (got["sums"] == SENT_F).all()
    assert (got["counts"] == SENT_I).all() and got["cost"].tolist() == [3.0, 4.0] and got["state"].tolist() == [1, 5]
    assert (s.ws == 0x5A).all().item()
    s = Step(x, c)                                                   # tol 1: |prev - cost| <= cost at the second step
    one = s.run(tol=1.0)
    assert one["state"].tolist() == [0, 1]
    two = s.run(tol=1.0)
    assert two["state"].tolist() == [1, 2] and two["cost"][1] == one["cost"][0]
    three = s.run(tol=1.0)
    assert all(np.array_equal(two[key], three[key]) for key in two)


# ---- k-means++ -------------------------------------------------------------------------------------------------------
class Pp:
    def __init__(self, x, k):
        from mdgen_amd.analysis import kmeans_pp_workspace_bytes
        self.x, self.k, self.n = _dev(x), k, len(x)
        self.bc, self.chosen = _guarded(k, torch.int64, SENT_I)
        self.bm, self.mind2 = _guarded(self.n, torch.float32, SENT_F)
        self.ws = torch.full((kmeans_pp_workspace_bytes(self.n, x.shape[1], k) + GUARD,), 0x5A, dtype=torch.uint8, device=_cuda())

    def run(self, u, r0, r1):
        from mdgen_amd.analysis import kmeans_pp_into
        kmeans_pp_into(self.x, self.k, u, r0, r1, self.chosen, self.mind2, self.ws[:-GUARD])
        torch.cuda.synchronize()
        _guard_ok(self.bc, self.k, SENT_I)
        _guard_ok(self.bm, self.n, SENT_F)
        assert (self.ws[-GUARD:] == 0x5A).all().item(), "workspace guard overwritten"
        return self.chosen.cpu().numpy().copy(), self.mind2.cpu().numpy().copy()


@pytest.mark.parametrize("n,d,k,seed", K.PP_CASES)
def test_kmeans_pp_round_by_round(n, d, k, seed):
    x, _ = K.inputs(n, d, k, seed)
    x64 = x.astype(np.float64)
    u = np.random.default_rng(K.PP_SEED).random(k)
    p = Pp(x, k)
    chosen, mind2 = p.run(u, 0, 1)
    assert chosen[0] == int(np.floor(u[0] * n)) and (chosen[1:] == SENT_I).all() and np.isposinf(mind2).all()
    ref, g, margin = np.full(n, np.inf), np.zeros(n), np.inf
    for r in range(1, k):
        chosen, mind2 = p.run(u, r, r + 1)
        row = x64[chosen[r - 1]]
        ref = np.minimum(ref, ((x64 - row) ** 2).sum(1))
        g = np.maximum(g, (d + 2) * K.EPS32 * ((np.abs(x64) + np.abs(row)) ** 2).sum(1))
        assert (np.abs(mind2.astype(np.float64) - ref) <= g).all(), r
        want, m = K.pp_next(mind2, u[r], n)                 # from the device's own values
        assert m >= K.PP_MARGIN, (r, m)
        assert chosen[r] == want, (r, chosen[r], want)
        assert (chosen[r + 1:] == SENT_I).all()
        margin = min(margin, m)
    print(f"k-means++ n {n} d {d} k {k}: smallest margin {margin:.3e}")
    assert len(set(chosen.tolist())) == k
    q = Pp(x, k)
    all_at_once, mind2_once = q.run(u, 0, k)
    assert np.array_equal(all_at_once, chosen) and np.array_equal(mind2_once, mind2), "one call differs from round by round"


def test_kmeans_pp_of_equal_points():
    n, k = 300, 4
    x = np.full((n, 3), 1.5, np.float32)
    u = np.random.default_rng(K.PP_SEED).random(k)
    chosen, mind2 = Pp(x, k).run(u, 0, k)
    assert chosen.tolist() == [int(np.floor(v * n)) for v in u] and (mind2 == 0).all()


# ---- the fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,seed", K.BLOB_CASES)
def test_kmeans_fit_of_blobs(n, d, k, seed):
    from mdgen_amd import analysis as A
    x = K.blobs(n, d, k, seed)
    got = A.kmeans_fit(_dev(x), k)
    assert list(got) == ["centers", "dim", "steps", "cost", "cost_history", "seed", "chosen"]
    assert got["centers"].dtype == np.float32 and got["centers"].shape == (k, d) and got["dim"] == d and got["seed"] == 137
    want = K.lloyd(x, x[got["chosen"]])                   # the restatement from the same initial centres
    assert want["steps"] == 3 and want["undecided"] == 0
    assert got["steps"] == want["steps"] and len(got["cost_history"]) == 3 and got["cost"] == got["cost_history"][-1]
    a = A.kmeans_assign(_dev(x), _dev(got["centers"])).cpu().numpy()
    assert np.array_equal(a, K.assign(x, want["centers"])[0])
    _, mags, counts = K.cluster_sums(x, a, k)
    bound = 2 * K.EPS32 * np.abs(want["centers"]) + K.SUM_RTOL * mags / counts[:, None]
    assert (np.abs(got["centers"].astype(np.float64) - want["centers"]) <= bound).all()
    chosen_ref, margin = K.pp(x, np.random.default_rng(137).random(k))
    print(f"blobs n {n} d {d} k {k}: k-means++ margin of the restatement {margin:.3e}, same choice {np.array_equal(chosen_ref, got['chosen'])}")


def test_kmeans_fit_of_a_cloud():
    from mdgen_amd import analysis as A
    n, d, k, seed = K.CLOUD_CASE
    x, _ = K.inputs(n, d, k, seed)
    got, again = A.kmeans_fit(_dev(x), k), A.kmeans_fit(_dev(x), k)
    for key in ("centers", "cost_history", "chosen"):
        assert np.array_equal(got[key], again[key]), "two fits gave other bits"
    assert got["steps"] == again["steps"] and 2 <= got["steps"] <= 100 and len(got["cost_history"]) == got["steps"]
    h = got["cost_history"]
    print(f"cloud: {got['steps']} steps, cost {h[0]:.6g} -> {h[-1]:.6g}")
    assert (h[1:] <= h[:-1] * (1 + 1e-6)).all()
    if got["steps"] < 100:
        assert abs(h[-2] - h[-1]) <= 1e-5 * h[-1]
    a = A.kmeans_assign(_dev(x), _dev(got["centers"])).cpu().numpy()
    check_assignment(x, got["centers"], a)
    short = A.kmeans_fit(_dev(x), k, max_iter=5)
    assert short["steps"] == 5 and np.array_equal(short["cost_history"], h[:5])
    with pytest.raises(ValueError, match="at least as many points"):
        A.kmeans_fit(_dev(x[:5]), k)


# ---- count matrices --------------------------------------------------------------------------------------------------
def run_count(dtraj, lag, k):
    from mdgen_amd.analysis import count_matrix_into
    bc, counts = _guarded(k * k, torch.int64, SENT_I)
    bd, dropped = _guarded(1, torch.int64, SENT_I)
    count_matrix_into(_dev(dtraj, np.int32), lag, k, counts, dropped)
    torch.cuda.synchronize()
    _guard_ok(bc, k * k, SENT_I)
    _guard_ok(bd, 1, SENT_I)
    return counts.cpu().numpy().reshape(k, k), int(dropped.cpu()[0])


def check_count(dtraj, lag, k):
    got, dropped = run_count(dtraj, lag, k)
    want, wdrop = K.count_matrix(dtraj, lag, k)
    assert np.array_equal(got, want) and dropped == wdrop
    assert got.sum() + dropped == max(len(dtraj) - lag, 0)
    again = run_count(dtraj, lag, k)
    assert np.array_equal(got, again[0]) and dropped == again[1]
    return got, dropped


@pytest.mark.parametrize("n,lag,k", K.COUNT_CASES)
def test_count_matrix(n, lag, k):
    got, dropped = check_count(K.dtraj_case(n, lag, k), lag, k)
    if lag >= n:
        assert got.sum() == 0 and dropped == 0
    elif n - lag > 1000:                                  # (the cases exercise both outcomes)
        assert dropped > 0 and got.sum() > 0


@pytest.mark.parametrize("k", [10, 110, 111, 256])       # LDS counters up to k = 110, global ones beyond
def test_count_matrix_of_one_state(k):
    n = 100003 if k == 10 else 4099
    got, dropped = check_count(np.full(n, 3, np.int32), 5, k)
    assert got[3, 3] == n - 5 and dropped == 0
    d = K.dtraj_case(4099, 7, k)
    check_count(d, 7, k)


def test_count_matrix_refusal_leaves_the_outputs_alone():
    from mdgen_amd._lib import MdgenError, launch, lib, ptr
    dev = _cuda()
    bc, counts = _guarded(4, torch.int64, SENT_I)
    bd, dropped = _guarded(1, torch.int64, SENT_I)
    d = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(MdgenError, match="lag must be >= 0"):
        launch(lib.mdgen_traj_count_matrix, d, 8, -1, 2, ptr(d), ptr(counts), ptr(dropped))
    with pytest.raises(MdgenError, match="k must be in 1 .."):
        launch(lib.mdgen_traj_count_matrix, d, 8, 1, 257, ptr(d), ptr(counts), ptr(dropped))
    torch.cuda.synchronize()
    assert (bc == SENT_I).all().item() and (bd == SENT_I).all().item()


# ---- end to end ------------------------------------------------------------------------------------------------------
MSM_KEYS = ["kmeans", "msm", "pcca", "cmsm", "traj_metastable_probs", "ref_metastable_probs", "msm_transition_matrix", "pcca_pi",
            "msm_pi", "traj_msm", "traj_transition_matrix", "traj_pi"]
ESTIMATOR_KEYS = ["lag", "active_set", "count_matrix", "transition_matrix", "pi"]


def _plain(v):
    if isinstance(v, dict):
        return all(type(key) is str and _plain(x) for key, x in v.items())
    return type(v) in (np.ndarray, int, float)


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(a, b) if a.dtype.kind in "iu" else np.abs(a - b).max() <= 1e-12)


def test_analyze_with_msm_against_the_host_chain():
    from mdgen_amd import analysis as A
    dev = _cuda()
    e = K.E2E
    aat, traj, ref = K.e2e_trajectories()
    kw = dict(nlag=200, ref_nlag=200, tica_lag=e["tica_lag"])
    mkw = dict(msm=True, msm_k=e["msm_k"], msm_states=e["msm_states"], md_msm_lag=e["md_msm_lag"], msm_lag=e["msm_lag"],
               kmeans_seed=e["kmeans_seed"])
    got = A.analyze(torch.from_numpy(traj).to(dev), ref, aat, **kw, **mkw)
    base = ["features", "JSD", "our_decorrelation", "md_decorrelation", "tica_model"]
    assert list(got) == base + MSM_KEYS
    assert all(_plain(got[key]) for key in MSM_KEYS)
    assert list(got["kmeans"]) == ["centers", "dim", "steps", "cost", "seed"] and got["kmeans"]["seed"] == e["kmeans_seed"]
    for key in ("msm", "cmsm", "traj_msm"):
        assert list(got[key]) == ESTIMATOR_KEYS, key
    assert got["msm"]["lag"] == got["cmsm"]["lag"] == e["md_msm_lag"] and got["traj_msm"]["lag"] == e["msm_lag"]
    assert list(got["pcca"]) == ["memberships", "metastable_assignments", "pi_coarse", "eigenvalues"]
    pickle.loads(pickle.dumps(got))
    # the stages before the host chain, on the device's own outputs: projection -> k-means -> discretisation
    dim = got["tica_model"]["dim"]
    a_traj, a_ref = A.featurize(torch.from_numpy(traj).to(dev), aat), A.featurize(torch.from_numpy(ref).to(dev), aat)
    y_ref, y_traj = (A.tica_transform(got["tica_model"], a, max(dim, 2))[:, :dim].contiguous() for a in (a_ref, a_traj))
    km = A.kmeans_fit(y_ref, e["msm_k"], seed=e["kmeans_seed"])
    assert np.array_equal(km["centers"], got["kmeans"]["centers"]) and km["steps"] == got["kmeans"]["steps"] < 100
    assert got["kmeans"]["dim"] == dim and got["kmeans"]["centers"].shape == (e["msm_k"], dim) and km["cost"] == got["kmeans"]["cost"]
    centers = _dev(km["centers"])
    d_ref, d_traj = (A.kmeans_assign(y, centers).cpu().numpy() for y in (y_ref, y_traj))
    check_assignment(y_ref.cpu().numpy(), km["centers"], d_ref)
    # ... and the host chain from those dtrajs, with NumPy counts
    want = K.host_chain(d_ref, d_traj, e["msm_k"], e["msm_states"], e["md_msm_lag"], e["msm_lag"])
    for key in ("msm", "cmsm", "traj_msm"):
        for part in ESTIMATOR_KEYS[1:]:
            assert _close(got[key][part], want[key][part]), (key, part)
    for part in ("memberships", "metastable_assignments", "pi_coarse", "eigenvalues"):
        assert _close(got["pcca"][part], want["pcca"][part]), part
    for key in MSM_KEYS[4:9] + MSM_KEYS[10:]:
        assert _close(got[key], want[key]), key
    assert len(got["msm"]["active_set"]) == e["msm_k"] and got["msm"]["count_matrix"].dtype == np.int64
    assert abs(got["traj_metastable_probs"].sum() - 1) <= 1e-12 and abs(got["ref_metastable_probs"].sum() - 1) <= 1e-12
    assert got["msm_transition_matrix"].shape == (3, 3) and np.abs(got["msm_transition_matrix"].sum(1) - 1).max() <= 1e-12
    assert abs(got["msm_pi"].sum() - 1) <= 1e-12 and abs(got["pcca_pi"].sum() - 1) <= 1e-12
    # without the sampled trajectory's MSM; and msm=False: the parent's result, key for key
    no_traj = A.analyze(torch.from_numpy(traj).to(dev), ref, aat, **kw, **mkw, traj_msm=False)
    assert list(no_traj) == base + MSM_KEYS[:9] and all(_close(no_traj[key], got[key]) for key in MSM_KEYS[4:9])
    tica = A.analyze(torch.from_numpy(traj).to(dev), ref, aat, **kw, tica=True)
    plain = A.analyze(torch.from_numpy(traj).to(dev), ref, aat, nlag=200, ref_nlag=200)
    assert list(tica) == base and list(plain) == base[:4]
    assert tica["JSD"] == got["JSD"] and tica["features"] == got["features"]
    assert all(np.array_equal(tica["tica_model"][key], got["tica_model"][key]) for key in tica["tica_model"])
    for key in ("our_decorrelation", "md_decorrelation"):
        assert all(np.array_equal(tica[key][lab], got[key][lab], equal_nan=True) for lab in tica[key])
        assert all(np.array_equal(plain[key][lab], got[key][lab], equal_nan=True) for lab in plain[key])
    assert all(plain["JSD"][key] == got["JSD"][key] for key in plain["JSD"])


def test_analyze_msm_refusals(capsys):
    from mdgen_amd import analysis as A
    dev = _cuda()
    aat = R.aatype_of("FLRH")
    traj, ref = R.peptide(300, aat, seed=30, walk=0.2), R.peptide(400, aat, seed=40, walk=0.2)
    t = torch.from_numpy(traj).to(dev)
    with pytest.raises(ValueError, match="no transition counts"):            # the MD trajectory is shorter than the MSM lag
        A.analyze(t, ref, aat, tica_lag=5, msm=True, msm_k=6, msm_states=2, md_msm_lag=400)
    with pytest.raises(ValueError, match="at least as many points"):
        A.analyze(t, ref[:50], aat, tica_lag=5, msm=True, msm_k=100, msm_states=2, md_msm_lag=2)
    with pytest.raises(ValueError, match="connected set"):                    # 200 microstates of 400 frames at lag 150
        A.analyze(t, ref, aat, tica_lag=5, msm=True, msm_k=200, msm_states=2, md_msm_lag=150)
    capsys.readouterr()
    got = A.analyze(t, ref, aat, tica_lag=5, msm=True, msm_k=3, msm_states=2, md_msm_lag=2, msm_lag=300, kmeans_seed=2, name="pX")
    assert "pX: no traj_msm entries" in capsys.readouterr().err              # only the sampled trajectory's MSM fails
    assert list(got)[-9:] == MSM_KEYS[:9]


def test_cli_analyze_peptide_sim_msm(tmp_path, capsys):
    """analyze_peptide_sim --msm --save on test_cli_analyze_peptide_sim's two peptides: the pickle holds analyze(..., msm=True) of
    what was read, and loads in a process that cannot import this package.  These 400-frame random walks rarely return: with seed
    2 the restatement finds pB's four microstates connected and only three of pA's, so both outcomes are met; the test holds
    whichever peptide is refused, as long as one is not."""
    from mdgen_amd import analyze_peptide_sim as cli
    from mdgen_amd.analysis import analyze
    from mdgen_amd.pdb import atom14_to_pdb, pdb_to_atom14
    dev = _cuda()
    names = {"pA": "FLRH", "pB": "AWKD"}
    out, data = tmp_path / "out", tmp_path / "data"
    out.mkdir()
    data.mkdir()
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\n" + "".join(f"{n},{s}\n" for n, s in names.items()))
    trajs = {}
    for i, (n, sq) in enumerate(names.items()):
        aat = R.aatype_of(sq)
        trajs[n] = R.peptide(300, aat, seed=30 + i, walk=0.2)
        np.save(data / f"{n}.npy", R.peptide(400, aat, seed=40 + i, walk=0.2).astype(np.float16))
    np.save(out / "pA.npy", trajs["pA"])
    atom14_to_pdb(trajs["pB"], R.aatype_of("AWKD"), str(out / "pB.pdb"))
    opts = ["--tica_lag", "5", "--msm_k", "4", "--msm_states", "2", "--md_msm_lag", "2", "--msm_lag", "1", "--kmeans_seed", "2"]
    capsys.readouterr()
    got = cli.main(["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--msm", "--save", "--truncate", "250"] + opts)
    err = capsys.readouterr().err
    code = ("import sys, pickle; sys.modules['mdgen_amd'] = None; d = pickle.load(open(sys.argv[1], 'rb')); "
            "print(list(d), [len(v) for v in d.values()])")
    r = subprocess.run([sys.executable, "-c", code, str(out / "out.pkl")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.startswith("['pA', 'pB']"), r.stderr
    saved = pickle.load(open(out / "out.pkl", "rb"))
    assert list(got) == list(saved) == ["pA", "pB"]
    read = {"pA": trajs["pA"], "pB": pdb_to_atom14(str(out / "pB.pdb"), R.aatype_of("AWKD"))}
    with_msm = 0
    for n, sq in names.items():
        refused = "msm" not in saved[n]
        assert refused == (f"{n}: no MSM entries" in err), (n, err)
        if refused:
            continue
        with_msm += 1
        want = analyze(torch.from_numpy(read[n][:250]).to(dev), np.load(data / f"{n}.npy"), R.aatype_of(sq), tica_lag=5, msm=True,
                       msm_k=4, msm_states=2, md_msm_lag=2, msm_lag=1, kmeans_seed=2)
        assert list(saved[n]) == list(want) and list(saved[n])[5:14] == MSM_KEYS[:9]
        assert saved[n]["JSD"] == want["JSD"] and saved[n]["kmeans"]["seed"] == 2 and saved[n]["kmeans"]["centers"].shape[0] == 4
        assert np.array_equal(saved[n]["kmeans"]["centers"], want["kmeans"]["centers"])
        for key in MSM_KEYS[4:9]:
            assert np.array_equal(saved[n][key], want[key]), key
        assert saved[n]["msm"]["lag"] == 2 and len(saved[n]["msm"]["active_set"]) == 4
        if "traj_msm" in saved[n]:
            assert saved[n]["traj_msm"]["lag"] == 1
    assert with_msm >= 1, err
    # --no_traj_msm acts
    got = cli.main(["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--msm", "--no_traj_msm", "--truncate", "250"]
                   + opts)
    assert all("traj_msm" not in v for v in got.values()) and any("cmsm" in v for v in got.values())


def test_sim_inference_analyze_msm(tmp_path, capsys):
    """sim_inference --synthetic --analyze --msm at test_sim_inference_analyze_tica's sizes (2 peptides, 50 frames, 3-frame MD
    files): the flag arrives -- three MD frames cannot carry 100 centres, so every peptide's MSM is refused, named on stderr, and the
    peptide keeps what --tica alone gives it."""
    from test_tica_gpu import _sim_inputs
    from mdgen_amd import sim_inference as cli
    from mdgen_amd.analyze_peptide_sim import analyze_one
    from mdgen_amd.geometry import restype_order
    names = {"FLRH": "FLRH", "AWKD": "AWKD"}
    data, split = _sim_inputs(tmp_path, names)
    common = ["--synthetic", "--data_dir", str(data), "--split", str(split), "--num_frames", "50", "--num_rollouts", "2",
              "--num_steps", "2", "--batch", "2", "--npy", "--analyze", "--tica_lag", "1"]
    out = tmp_path / "out"
    capsys.readouterr()
    cli.main(common + ["--out_dir", str(out), "--msm"])
    err = capsys.readouterr().err
    got = pickle.load(open(out / "analysis.pkl", "rb"))
    assert list(got) == list(names)
    for n, sq in names.items():
        assert f"{n}: no MSM entries" in err, err
        traj = torch.from_numpy(np.load(out / f"{n}.npy")).to(_cuda())
        want = analyze_one(n, traj, np.load(data / f"{n}.npy"), np.array([restype_order[c] for c in sq]), tica=True, tica_lag=1)
        assert list(got[n]) == list(want) and got[n]["JSD"] == want["JSD"] and "kmeans" not in got[n]
