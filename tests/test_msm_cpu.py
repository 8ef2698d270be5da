"""The k-means / MSM chain without a device: the entry points' bindings and refusals, mdgen_amd/msm.py (connected set, reversible
maximum likelihood, PCCA+, the least-flux pair) against their defining equations, the command line, and tests/msm_ref.py -- the
restatement the kernels are held against on the GPU: its cases stay inside the gates its docstring derives."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mdgen_traj_kmeans_assign": ["n", "d", "k", "x", "centers", "assign", "dist2", "stream"],
       "mdgen_traj_kmeans_step_workspace_bytes": ["n", "d", "k", "bytes"],
       "mdgen_traj_kmeans_step": ["n", "d", "k", "x", "centers", "assign", "sums", "counts", "cost", "state", "tol", "workspace",
                                  "workspace_bytes", "stream"],
       "mdgen_traj_kmeans_pp_workspace_bytes": ["n", "d", "k", "bytes"],
       "mdgen_traj_kmeans_pp": ["n", "d", "k", "x", "u", "r0", "r1", "chosen", "mind2", "workspace", "workspace_bytes", "stream"],
       "mdgen_traj_count_matrix": ["n", "lag", "k", "dtraj", "counts", "dropped", "stream"]}


def test_header_exports_and_binding_agree():
    import mdgen_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    kind = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    for name, want in NEW.items():
        decl = re.search(r"int32_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == want, name
        kinds = [ctypes.c_void_p if "*" in p else kind[p.split()[0]] for p in params]
        got = list(getattr(L.lib, name).argtypes)
        if name.endswith("workspace_bytes"):
            assert got[:3] == kinds[:3] and got[3] is ctypes.POINTER(ctypes.c_size_t)
        else:
            assert got == kinds, name
        assert L.EXPORTS.count(name) == 1 and getattr(L.lib, name).restype is ctypes.c_int32
    assert "#define MDGEN_ABI_VERSION 8" in hdr and L.lib.mdgen_abi_version() == L.ABI_VERSION == 8   # additions only


def test_refusals_without_a_device():
    """Every refusal is decided on the host, the shape before the pointers: null pointers are enough, nothing is dereferenced
    (u, a host array, is read only once the shape has passed)."""
    import mdgen_amd._lib as L
    lib, err = L.lib, L.lib.mdgen_last_error
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    b = ctypes.c_size_t()
    u = np.array([0.5, 0.25], np.float64)
    for d, k in ((0, 1), (129, 1), (1, 0), (1, 257)):
        assert lib.mdgen_traj_kmeans_assign(5, d, k, None, None, None, None, None) == -2, (d, k)
        assert b"must be in 1 .." in err()
        assert lib.mdgen_traj_kmeans_step(5, d, k, None, None, None, None, None, None, None, 1e-5, None, 0, None) == -2
        assert lib.mdgen_traj_kmeans_pp(5, d, k, None, None, 0, 0, None, None, None, 0, None) == -2
        assert lib.mdgen_traj_kmeans_step_workspace_bytes(5, d, k, ctypes.byref(b)) == -2
        assert lib.mdgen_traj_kmeans_pp_workspace_bytes(5, d, k, ctypes.byref(b)) == -2
    assert lib.mdgen_traj_kmeans_assign(0, 1, 1, None, None, None, None, None) == -2
    assert lib.mdgen_traj_kmeans_assign(5, 1, 1, None, None, None, None, None) == -1 and b"null" in err()
    assert lib.mdgen_traj_kmeans_step(5, 2, 2, p, p, p, p, p, p, p, -1.0, p, 1 << 20, None) == -2 and b"tol" in err()
    assert lib.mdgen_traj_kmeans_step(5, 2, 2, p, p, p, p, p, p, p, float("nan"), p, 1 << 20, None) == -2
    assert lib.mdgen_traj_kmeans_step(5, 2, 2, p, p, p, p, p, p, None, 1e-5, p, 1 << 20, None) == -1
    assert lib.mdgen_traj_kmeans_step_workspace_bytes(5, 2, 2, ctypes.byref(b)) == 0 and b.value > 0
    assert lib.mdgen_traj_kmeans_step(5, 2, 2, p, p, p, p, p, p, p, 1e-5, p, b.value - 1, None) == -3 and b"workspace" in err()
    assert lib.mdgen_traj_kmeans_pp_workspace_bytes(5, 2, 2, ctypes.byref(b)) == 0 and b.value == 8
    assert lib.mdgen_traj_kmeans_pp(5, 2, 2, p, u.ctypes.data, 0, 2, p, p, p, b.value - 1, None) == -3
    for r0, r1 in ((-1, 1), (2, 1), (0, 3)):
        assert lib.mdgen_traj_kmeans_pp(5, 2, 2, p, u.ctypes.data, r0, r1, p, p, p, 8, None) == -2 and b"rounds" in err()
    for bad in (1.0, -0.1, float("nan")):
        assert lib.mdgen_traj_kmeans_pp(5, 2, 2, p, np.array([0.5, bad]).ctypes.data, 0, 2, p, p, p, 8, None) == -2 and b"u[1]" in err()
    assert lib.mdgen_traj_kmeans_pp(5, 2, 2, p, None, 0, 2, p, p, p, 8, None) == -1
    assert lib.mdgen_traj_count_matrix(5, -1, 2, None, None, None, None) == -2 and b"lag" in err()
    assert lib.mdgen_traj_count_matrix(0, 1, 2, None, None, None, None) == -2
    assert lib.mdgen_traj_count_matrix(5, 1, 0, None, None, None, None) == -2
    assert lib.mdgen_traj_count_matrix(5, 1, 257, None, None, None, None) == -2
    assert lib.mdgen_traj_count_matrix(5, 1, 2, None, None, None, None) == -1
    # the reference's size fits a device: 10^6 frames, 100 centres, 10 components
    assert lib.mdgen_traj_kmeans_step_workspace_bytes(1000000, 10, 100, ctypes.byref(b)) == 0 and b.value < 1 << 24
    assert lib.mdgen_traj_kmeans_step_workspace_bytes(1000000, 128, 256, ctypes.byref(b)) == 0 and b.value < 1 << 25


def test_wrappers_refuse_before_a_device_is_needed():
    from mdgen_amd import analysis as A
    for n, d, k in ((0, 1, 1), (5, 0, 1), (5, 129, 1), (5, 1, 0), (5, 1, 257)):
        with pytest.raises(ValueError):
            A._check_kmeans_shape(n, d, k)
    with pytest.raises(Exception, match="GPU only"):
        A.kmeans_fit(np.zeros((8, 2), np.float32), 2)


# ---- the host estimators ---------------------------------------------------------------------------------------------
def test_largest_connected_set():
    from mdgen_amd.msm import largest_connected_set
    C = np.zeros((8, 8), np.int64)
    for a, b in ((1, 3), (3, 5), (5, 1)):         # a cycle of three
        C[a, b] = 2
    for a, b in ((0, 2), (2, 4), (4, 0)):         # a cycle of three that contains the lowest state: it wins the tie
        C[a, b] = 1
    C[6, 1] = 5                                   # 6 is transient: it reaches a cycle and nothing returns
    C[7, 7] = 9                                   # 7 only itself
    got = largest_connected_set(C)
    assert got.dtype == np.int64 and got.tolist() == [0, 2, 4]
    C[4, 6] = 1
    C[6, 0] = 1                                   # now {0, 2, 4, 6} and, through 6 -> 1 but not back, still not the other cycle
    assert largest_connected_set(C).tolist() == [0, 2, 4, 6]
    C[5, 6] = 1                                   # ... and back: seven states
    assert largest_connected_set(C).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert largest_connected_set(np.zeros((3, 3))).tolist() == [0]
    chain = np.diag(np.ones(255), 1) + np.diag(np.ones(255), -1)      # 256 states in a line: the closure needs 8 squarings
    assert largest_connected_set(chain).tolist() == list(range(256))


@pytest.fixture(scope="module")
def chain_msm():
    from mdgen_amd import msm as M
    C, dropped = K.count_matrix(K.three_well_chain(), 5, 30)
    assert dropped == 0
    return C, M.estimate_msm(C, 5)


def test_mle_reversible(chain_msm):
    from mdgen_amd import msm as M
    C, m = chain_msm
    assert list(m) == ["lag", "active_set", "count_matrix", "transition_matrix", "pi"] and m["lag"] == 5
    assert m["active_set"].tolist() == list(range(30)) and np.array_equal(m["count_matrix"], C)
    T, pi = m["transition_matrix"], m["pi"]
    assert np.abs(T.sum(1) - 1).max() <= 1e-12 and abs(pi.sum() - 1) <= 1e-12 and (T >= 0).all() and (pi > 0).all()
    flux = pi[:, None] * T
    assert np.abs(flux - flux.T).max() <= 1e-12
    assert np.abs(pi @ T - pi).max() <= 1e-12
    # the fixed point: X_ij (c_i / x_i + c_j / x_j) = S_ij, with X = diag(x) T for any scale of x
    S, c = (C + C.T).astype(np.float64), C.sum(1).astype(np.float64)
    lhs = flux * (c / pi)[:, None] + flux * (c / pi)[None, :]
    scale = S.sum() / lhs.sum()
    assert abs(scale - 1) <= 1e-6 * 30      # (sum X (c_i/x_i + c_j/x_j) = 2 sum c = sum S: the scale is 1)
    assert np.abs(lhs - S).max() <= 1e-6 * S.max()
    T2, pi2, it = M.mle_reversible(C)
    assert np.array_equal(T2, T) and np.array_equal(pi2, pi) and 100 < it < 100000
    # a symmetric count matrix is its own fixed point
    Cs = C + C.T
    Ts, pis, _ = M.mle_reversible(Cs)
    assert np.abs(Ts - Cs / Cs.sum(1, keepdims=True)).max() <= 1e-10 and np.abs(pis - Cs.sum(1) / Cs.sum()).max() <= 1e-10
    with pytest.raises(ValueError, match="no counts"):
        M.mle_reversible(np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0]]))
    with pytest.raises(ValueError, match="did not converge"):
        M.mle_reversible(C, maxiter=3)
    one = M.estimate_msm(np.array([[0, 3], [0, 4]]), 2)               # 0 -> 1 only: two sets of one state, the lower wins the tie
    assert one["active_set"].tolist() == [0] and one["transition_matrix"].tolist() == [[1.0]] and one["pi"].tolist() == [1.0]


def test_pcca(chain_msm):
    from mdgen_amd import msm as M
    T, pi, blocks = K.block_chain()
    flux = pi[:, None] * T
    assert np.abs(flux - flux.T).max() <= 1e-15
    p = M.pcca(T, pi, 3)
    assert list(p) == ["memberships", "metastable_assignments", "pi_coarse", "eigenvalues"]
    chi, meta = p["memberships"], p["metastable_assignments"]
    assert chi.shape == (12, 3) and (chi >= 0).all() and (chi <= 1).all() and np.abs(chi.sum(1) - 1).max() <= 1e-12
    assert meta.dtype == np.int64 and sorted(len(set(meta[b])) for b in blocks) == [1, 1, 1]        # a block is in one set ...
    assert len({int(meta[b[0]]) for b in blocks}) == 3                                                # ... and the sets differ
    assert chi.max(1).min() > 0.99                                                                    # nearly crisp at eps = 1e-3
    assert np.abs(p["pi_coarse"] - pi @ chi).max() == 0 and abs(p["pi_coarse"].sum() - 1) <= 1e-12
    assert np.all(np.diff(p["eigenvalues"]) <= 0) and abs(p["eigenvalues"][0] - 1) <= 1e-12
    # the three-well chain: three contiguous sets, memberships inside [0, 1] after the clip
    _, m = chain_msm
    q = M.pcca(m["transition_matrix"], m["pi"], 3)
    meta = q["metastable_assignments"]
    assert len(set(meta.tolist())) == 3 and (np.diff(meta) != 0).sum() == 2
    assert (q["memberships"] >= 0).all() and (q["memberships"] <= 1).all() and np.abs(q["memberships"].sum(1) - 1).max() <= 1e-12
    assert M.pcca(T, pi, 1)["metastable_assignments"].tolist() == [0] * 12
    with pytest.raises(ValueError):
        M.pcca(T, pi, 13)


def test_least_flux_pair():
    from mdgen_amd.msm import least_flux_pair
    T = np.array([[0.90, 0.10, 0.00], [0.05, 0.90, 0.05], [0.00, 0.20, 0.80]])
    pi = np.array([0.25, 0.5, 0.25])           # flux = T * pi[None, :]: the smallest entry >= 1e-7 is T[1, 0] pi[0] = 0.0125
    cmsm = {"transition_matrix": T, "pi": pi, "active_set": np.array([0, 2, 5])}
    assert least_flux_pair(cmsm) == (2, 0)
    T2 = T.copy()
    T2[0, 2], T2[0, 1] = 1e-8, 0.1 - 1e-8      # below 1e-7: not chosen
    assert least_flux_pair({"transition_matrix": T2, "pi": pi, "active_set": np.array([0, 2, 5])}) == (2, 0)
    T2[0, 2], T2[0, 1] = 1e-6, 0.1 - 1e-6      # above: chosen
    assert least_flux_pair({"transition_matrix": T2, "pi": pi, "active_set": np.array([0, 2, 5])}) == (0, 5)
    assert np.array_equal(cmsm["transition_matrix"], T)      # the argument is not written


def test_msm_imports_without_torch_or_scipy():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; sys.modules['scipy'] = None; import mdgen_amd.msm as M; "
            "import numpy as np; print(M.largest_connected_set(np.ones((2, 2))).tolist())")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "[0, 1]", r.stderr


# ---- the command line ------------------------------------------------------------------------------------------------
def test_cli_options(tmp_path, capsys):
    from mdgen_amd import analyze_peptide_sim as cli
    from mdgen_amd import sim_inference as sim
    p = cli.build_parser()
    a = p.parse_args(["--pdbdir", "x", "--msm"])
    assert a.msm and not a.no_msm and (a.msm_k, a.msm_states, a.md_msm_lag, a.msm_lag, a.kmeans_seed) == (100, 10, 1000, 10, 137)
    assert cli.msm_options(a) == dict(msm=True, msm_k=100, msm_states=10, md_msm_lag=1000, msm_lag=10, traj_msm=True, kmeans_seed=137)
    a = p.parse_args(["--pdbdir", "x", "--msm", "--msm_k", "12", "--msm_states", "3", "--md_msm_lag", "5", "--msm_lag", "2",
                      "--kmeans_seed", "7", "--no_traj_msm"])
    assert cli.msm_options(a) == dict(msm=True, msm_k=12, msm_states=3, md_msm_lag=5, msm_lag=2, traj_msm=False, kmeans_seed=7)
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--pdbdir", "x", "--msm", "--no_msm"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    nowhere = str(tmp_path / "nowhere")
    with pytest.raises(SystemExit) as e:       # neither flag: refused as before, before anything is read
        cli.main(["--pdbdir", nowhere, "--data_dir", nowhere, "--split", nowhere + ".csv"])
    assert e.value.code == 2 and "pyemma" in capsys.readouterr().err
    with pytest.raises(FileNotFoundError):     # --msm passes the refusal and goes on to read the split
        cli.main(["--msm", "--pdbdir", nowhere, "--data_dir", nowhere, "--split", nowhere + ".csv"])
    s = sim.build_parser().parse_args(["--data_dir", "x", "--analyze", "--msm", "--msm_k", "12"])
    assert s.msm and cli.msm_options(s)["msm_k"] == 12 and cli.msm_options(s)["traj_msm"] is True


# ---- the restatement's cases stay inside their gates -------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,seed", K.ASSIGN_CASES)
def test_assignment_cases_are_mostly_decided(n, d, k, seed):
    x, c = K.inputs(n, d, k, seed)
    arg, dmin, decided, g = K.assign(x, c)
    share = float((~decided).mean())
    print(f"assign n {n} d {d} k {k}: {int((~decided).sum())} undecided ({share:.4%})")
    assert share <= K.UNDECIDED_CAP
    assert np.array_equal(arg, np.argmin(K.dist2(x, c), axis=1)) and (g > 0).all()
    # the same chain in fp32 (a NumPy evaluation, its own order) stays inside the gate: the gate is no tighter than fp32 allows
    d32 = ((x[:, None, :] - c[None, :8, :]) ** 2).sum(-1, dtype=np.float32)
    assert (np.abs(d32.astype(np.float64) - K.dist2(x, c[:8])) <= g[:, None]).all()


@pytest.mark.parametrize("n,d,k,seed", K.PP_CASES)
def test_kmeans_pp_cases_have_a_margin(n, d, k, seed):
    x, _ = K.inputs(n, d, k, seed)
    chosen, margin = K.pp(x, np.random.default_rng(K.PP_SEED).random(k))
    print(f"k-means++ n {n} d {d} k {k}: smallest margin {margin:.3e}")
    assert margin >= 100 * K.PP_MARGIN and len(set(chosen.tolist())) == k and 0 <= chosen.min() and chosen.max() < n


def test_pp_next_rules():
    w = np.array([0.0, 1.0, 0.0, 3.0], np.float32)
    assert K.pp_next(w, 0.0, 4)[0] == 1 and K.pp_next(w, 0.2499, 4)[0] == 1 and K.pp_next(w, 0.25, 4)[0] == 3
    assert K.pp_next(np.zeros(4, np.float32), 0.6, 4) == (2, np.inf)
    assert abs(K.pp_next(w, 0.625, 4)[1] - 0.5) < 1e-12


@pytest.mark.parametrize("n,d,k,seed", K.BLOB_CASES)
def test_blob_cases_converge_with_every_point_decided(n, d, k, seed):
    r = K.fit(K.blobs(n, d, k, seed), k)
    h = r["cost_history"]
    assert r["steps"] == 3 and r["undecided"] == 0 and h[-2] == h[-1]
    assert len(np.unique(r["assign"])) == k


def test_cloud_case_is_long():
    n, d, k, seed = K.CLOUD_CASE
    r = K.fit(K.inputs(n, d, k, seed)[0], k)
    assert 10 < r["steps"] < 100 and np.all(np.diff(r["cost_history"]) <= 0)


def test_count_matrix_restatement():
    d = np.array([0, 1, 1, 2, -1, 0, 3, 1], np.int32)
    C, dropped = K.count_matrix(d, 1, 3)
    want = np.zeros((3, 3), np.int64)
    for a, b in zip(d[:-1], d[1:]):
        if 0 <= a < 3 and 0 <= b < 3:
            want[a, b] += 1
    assert np.array_equal(C, want) and dropped == 4 and C.sum() + dropped == 7
    assert K.count_matrix(d, 8, 3)[0].sum() == 0 and K.count_matrix(d, 0, 3)[0].trace() == 6
    for n, lag, k in K.COUNT_CASES:
        dt = K.dtraj_case(n, lag, k)
        assert dt.min() >= -1 and dt.max() <= k


def test_end_to_end_case_has_every_microstate_active():
    """The GPU end-to-end test's sizes and seeds (K.E2E) are chosen so that the restatement finds all 12 microstates in the MSM's
    connected set, three metastable sets in use, and a sampled-trajectory MSM."""
    e = K.E2E
    d_ref, d_traj, km = K.e2e_restatement()
    assert len(np.unique(d_ref)) == e["msm_k"] and km["steps"] < 100
    h = K.host_chain(d_ref, d_traj, e["msm_k"], e["msm_states"], e["md_msm_lag"], e["msm_lag"])
    assert len(h["msm"]["active_set"]) == e["msm_k"]
    assert len(set(h["pcca"]["metastable_assignments"].tolist())) == e["msm_states"]
    assert h["cmsm"]["active_set"].tolist() == [0, 1, 2] and len(h["traj_msm"]["active_set"]) >= 2
    assert abs(h["ref_metastable_probs"].sum() - 1) <= 1e-12 and abs(h["traj_metastable_probs"].sum() - 1) <= 1e-12
    # the lumped count matrix M' C M is the count matrix of the lumped dtraj
    C, _ = K.count_matrix(d_ref, e["md_msm_lag"], e["msm_k"])
    lump = np.zeros((e["msm_k"], e["msm_states"]), np.int64)
    lump[np.arange(e["msm_k"]), h["pcca"]["metastable_assignments"]] = 1
    assert np.array_equal(lump.T @ C @ lump, h["cmsm"]["count_matrix"])
