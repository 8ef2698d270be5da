"""Transition paths without a device: mdgen_tp_sample's binding and refusals, the host estimators of mdgen_amd/msm.py (bridge_table,
tp_likelihood, state_probs, bridge_exact, tps_endpoints) against the reference's loop forms and brute-force enumeration, the
statistics of the restated sampler against the exact expectations, and the two command lines.  tests/tps_ref.py derives the gates."""
import ctypes
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tps_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ["n_samples", "N", "k", "Ta", "Ba", "start", "end", "seed", "stream_id", "sample_base", "kb", "Tb", "Bb", "phi", "paths",
          "prob", "stream"]


def test_header_exports_and_binding_agree():
    import mdgen_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    kind = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    decl = re.search(r"int32_t mdgen_tp_sample\((.*?)\);", hdr, re.S).group(1)
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == PARAMS
    assert list(L.lib.mdgen_tp_sample.argtypes) == [ctypes.c_void_p if "*" in p else kind[p.split()[0]] for p in params]
    assert L.EXPORTS.count("mdgen_tp_sample") == 1 and L.lib.mdgen_tp_sample.restype is ctypes.c_int32
    assert "#define MDGEN_ABI_VERSION 8" in hdr and L.lib.mdgen_abi_version() == L.ABI_VERSION == 8   # an addition only
    from mdgen_amd import build
    assert "k_tps.hip" in build.SOURCES and "-ffp-contract=off" in build.flags_for("k_tps.hip")


def test_refusals_without_a_device():
    """Every refusal is decided on the host, the shape before the pointers: a 64-byte buffer stands for every device pointer and is
    never read (only phi, a host array, is)."""
    import mdgen_amd._lib as L
    lib, err = L.lib, L.lib.mdgen_last_error
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    phi = np.array([0, 1, 1], np.int32)

    def call(n=5, N=4, k=3, Ta=p, Ba=p, start=0, end=2, kb=0, Tb=None, Bb=None, ph=None, paths=p, prob=None):
        return lib.mdgen_tp_sample(n, N, k, Ta, Ba, start, end, 1, 2, 0, kb, Tb, Bb, ph, paths, prob, None)
    for kw in (dict(n=0), dict(n=-3), dict(N=1), dict(N=4097), dict(k=0), dict(k=65), dict(kb=-1), dict(kb=65), dict(start=-1),
               dict(start=3), dict(end=-1), dict(end=3)):
        assert call(**kw) == -2, kw
        assert call(Ta=None, Ba=None, paths=None, **kw) == -2, kw        # the shape first
    assert call(start=3) == -2 and b"outside the 3 states" in err()
    for kw in (dict(Ta=None), dict(Ba=None), dict(paths=None)):
        assert call(**kw) == -1 and b"null" in err(), kw
    full = dict(kb=2, Tb=p, Bb=p, ph=phi.ctypes.data, prob=p)
    for key in ("Tb", "Bb", "ph", "prob"):
        assert call(**{**full, key: None}) == -1, key
    for bad in (-1, 2):
        phi2 = np.array([0, bad, 1], np.int32)
        assert call(**{**full, "ph": phi2.ctypes.data}) == -2 and b"phi[1]" in err()
    assert call(**{**full, "kb": 1}) == -2 and b"phi[1] = 1" in err()     # the same phi no longer fits one scoring state


def test_wrappers_refuse_before_a_device_is_needed():
    from mdgen_amd import analysis as A
    for n, N, k, s, e in ((0, 4, 3, 0, 1), (5, 1, 3, 0, 1), (5, 4097, 3, 0, 1), (5, 4, 0, 0, 0), (5, 4, 65, 0, 1), (5, 4, 3, 3, 1),
                          (5, 4, 3, 0, -1)):
        with pytest.raises(ValueError):
            A._check_tp_shape(n, N, k, s, e)
    T = np.array([[1.0, 0.0], [0.5, 0.5]])                 # state 0 never leaves: 1 cannot be reached
    with pytest.raises(ValueError, match="not reachable in N - 1 steps"):
        A.tp_sample(T, 0, 1, 5, 10, 1, 0)
    with pytest.raises(ValueError, match="phi"):
        A.tp_sample(T, 1, 0, 5, 10, 1, 0, score=(T, [0, 2]))


# ---- the restatement itself ------------------------------------------------------------------------------------------
def test_uniform_is_the_projects_generator():
    import mdgen_amd._lib as L
    from mdgen_amd.philox import bridge_uniform
    samples = np.array([0, 1, 999, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17, 2 ** 64 - 1], np.uint64)
    for seed, stream, t in ((0, 0, 1), (137, 3, 9), (2 ** 63 + 5, 2 ** 32 - 1, 4095)):
        u = R.uniform(seed, stream, samples, t)
        assert np.array_equal(u, bridge_uniform(seed, stream, samples, t)) and (u >= 0).all() and (u < 1).all()
        for i, s in enumerate(samples.tolist()):
            w = L.philox([s & 0xFFFFFFFF, s >> 32, t, stream], [seed & 0xFFFFFFFF, seed >> 32])     # csrc/philox.h on the host
            assert u[i] == ((int(w[0]) >> 5) * 2 ** 26 + (int(w[1]) >> 6)) * 2.0 ** -53
    u = R.uniform(1, 0, np.arange(200000, dtype=np.uint64), 1)
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * 200000) and len(np.unique(u)) == 200000


def test_draw_rule():
    """Hand cases of the rule: the smallest j with c_j > u c_{k-1}; pinned ends; a dead path holds -1 from the dead step on."""
    from mdgen_amd.msm import bridge_table
    Ta = np.array([[0.0, 1.0, 0.0], [0.0, 0.5, 0.5], [0.0, 0.0, 1.0]])       # 0 -> 1 is forced
    p = R.sample(Ta, bridge_table(Ta, 2, 4), 0, 2, 50, 3, 0)
    assert (p[:, 0] == 0).all() and (p[:, 1] == 1).all() and (p[:, 3] == 2).all() and set(p[:, 2].tolist()) == {1, 2}
    u = R.uniform(3, 0, np.arange(50, dtype=np.uint64), 2)
    assert np.array_equal(p[:, 2], np.where(0.25 > u * 0.75, 1, 2))           # from 1: w = Ta[1] B[1] = (0, .25, .5), c = (0, .25, .75)
    dead = R.sample(Ta, bridge_table(Ta, 0, 4), 1, 0, 3, 3, 0)                # state 0 cannot be reached from 1
    assert dead[:, 0].tolist() == [1, 1, 1] and (dead[:, 1:] == -1).all()
    for n, N, k, z in R.PATH_CASES:
        Ta, s, e = R.path_case(n, N, k, z)
        assert bridge_table(Ta, e, N)[N - 1, s] > 0 and abs((Ta == 0).mean() - z * (1 - 1 / k)) < 0.12, (n, N, k)


# ---- the host estimators ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 11, 101])
def test_bridge_table(N):
    from mdgen_amd.msm import bridge_table
    for k, seed, z in ((1, 0, 0.0), (3, 1, 0.3), (10, 2, 1 / 3)):
        T = R.chain(k, seed, z)
        for end in (0, k - 1):
            B, want = bridge_table(T, end, N), R.bridge_table(T, end, N)
            assert B.shape == (N, k) and B.dtype == np.float64
            assert np.allclose(B, want, rtol=1e-12, atol=0) and B[0].tolist() == [float(i == end) for i in range(k)]
    with pytest.raises(ValueError):
        bridge_table(np.ones((2, 3)), 0, 4)
    with pytest.raises(ValueError):
        bridge_table(np.eye(2), 2, 4)


def test_tp_likelihood():
    from mdgen_amd.msm import tp_likelihood
    T = R.chain(6, 3, 0.3)
    g = np.random.default_rng(0)
    tp = g.integers(0, 6, size=(200, 11))
    tp[1:, -1] = tp[0, -1]
    got, want = tp_likelihood(tp, T), R.likelihood_loop(tp, T)
    assert got.shape == (200, 10) and np.allclose(got, want, rtol=1e-12, atol=0)
    zero = np.argwhere(T == 0)
    assert len(zero) and (got == 0).any() and (got > 0).any()                 # random paths cross zero transitions
    # a path through a zero transition: that factor is 0 (0 * B / B, or 0 / 0 -> NaN -> 0)
    a, b = zero[0]
    path = np.array([[a, b, tp[0, -1]]])
    assert tp_likelihood(path, T)[0, 0] == 0 and R.likelihood_loop(path, T)[0, 0] == 0
    # an unreachable end: state 0 is absorbing, every factor towards state 1 is 0 / 0
    Tabs = np.array([[1.0, 0.0], [0.5, 0.5]])
    stuck = np.array([[0, 0, 0, 1], [1, 1, 1, 1]])
    got = tp_likelihood(stuck, Tabs)
    assert np.array_equal(got, R.likelihood_loop(stuck, Tabs)) and got[0].tolist() == [0, 0, 0] and np.allclose(got[1], 1.0)
    # the tp[0, -1] rule: every row is scored towards the FIRST row's end state, whatever its own
    mixed = tp.copy()
    mixed[5:, -1] = (tp[0, -1] + 1) % 6
    got, want = tp_likelihood(mixed, T), R.likelihood_loop(mixed, T)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    other = mixed.copy()
    other[0] = mixed[5]                                                       # another first row: another end state, other values
    assert not np.allclose(tp_likelihood(other, T)[1:5], got[1:5])
    with pytest.raises(ValueError):
        tp_likelihood(np.zeros((3, 1), int), T)


def test_state_probs():
    from mdgen_amd.msm import state_probs
    tp = np.array([[0, 3, 3, 9], [0, 0, 1, 9]])
    got = state_probs(tp)
    assert got.shape == (10,) and np.array_equal(got, R.state_probs_loop(tp)) and got[0] == 3 / 8 and got.sum() == 1
    assert state_probs(tp, 4).shape == (10,) and state_probs(tp[:, :3], 12).shape == (12,)      # minlength, as np.bincount


@pytest.mark.parametrize("k,N", [(3, 5), (4, 6)])
def test_bridge_exact_against_enumeration(k, N):
    from mdgen_amd.msm import bridge_exact
    Ta, Tb = R.chain(k, 10 + k, 0.3), R.chain(k + 1, 20 + k, 0.3)
    phi = np.array([(2 * i + 1) % (k + 1) for i in range(k)])                  # not the identity, into a larger chain
    assert (Ta == 0).any() and (Tb == 0).any()
    n_checked = 0
    for start in range(k):
        for end in range(k):
            want = R.enumerate_bridge(Ta, start, end, N, Tb, phi)
            if not want["Z"] > 0:
                continue
            got = bridge_exact(Ta, start, end, N, Tb, phi)
            assert abs(got["Z"] - want["Z"]) <= 1e-12 * want["Z"]
            assert np.abs(got["occupancy"] - want["occupancy"]).max() <= 1e-12 and abs(got["occupancy"].sum() - 1) <= 1e-12
            for key in ("prob", "valid_rate"):
                assert abs(got[key] - want[key]) <= 1e-12 * max(want[key], 1e-300), (key, start, end)
            if want["valid_rate"] > 0:
                assert abs(got["valid_prob"] - want["valid_prob"]) <= 1e-12 * want["valid_prob"]
            else:
                assert np.isnan(got["valid_prob"]) and np.isnan(want["valid_prob"]) and got["prob"] == 0
            n_checked += 1
    assert n_checked >= k * k - 2
    assert list(bridge_exact(Ta, 0, 1, N)) == ["Z", "occupancy"]
    with pytest.raises(ValueError, match="end state not reachable in N - 1 steps"):
        bridge_exact(np.array([[1.0, 0.0], [0.5, 0.5]]), 0, 1, N)


def test_sampler_statistics_against_the_exact_expectations():
    """40 000 paths of the restated sampler against `bridge_exact`: the gates are tests/tps_ref.py's Monte-Carlo bounds."""
    from mdgen_amd.msm import bridge_exact, bridge_table, state_probs, tp_likelihood
    S = R.STAT_CASE
    k, N, n = S["k"], S["N"], S["n"]
    Ta, Tb = R.chain(k, S["seed_a"], S["zero_a"]), R.chain(k, S["seed_b"], S["zero_b"])
    phi = np.array(S["phi"])
    ex = bridge_exact(Ta, S["start"], S["end"], N, Tb, phi)
    print(f"exact: valid rate {ex['valid_rate']:.5f} prob {ex['prob']:.4e} occupancy {np.round(ex['occupancy'], 4)}")
    assert 0.2 < ex["valid_rate"] < 0.8                                        # the check is not vacuous
    paths = R.sample(Ta, bridge_table(Ta, S["end"], N), S["start"], S["end"], n, S["seed"], S["stream"])
    assert paths.min() >= 0 and (paths[:, 0] == S["start"]).all() and (paths[:, -1] == S["end"]).all()
    assert (Ta[paths[:, :-1], paths[:, 1:]] > 0).all()                         # no path takes a forbidden step
    gate = 5.0 / (2.0 * np.sqrt(n))
    occ = state_probs(paths, k)
    like = tp_likelihood(phi[paths], Tb).prod(-1)
    rate = float((like > 0).mean())
    se = float(like.std(ddof=1) / np.sqrt(n))
    print(f"sampled: valid rate {rate:.5f} prob {like.mean():.4e} +- {se:.1e} occupancy error {np.abs(occ - ex['occupancy']).max():.2e} "
          f"(gate {gate:.2e})")
    assert np.abs(occ - ex["occupancy"]).max() <= gate
    assert abs(rate - ex["valid_rate"]) <= gate
    assert abs(like.mean() - ex["prob"]) <= 5 * se


def test_tps_endpoints():
    from mdgen_amd.msm import least_flux_pair, tps_endpoints
    T = np.array([[0.90, 0.10, 0.00], [0.05, 0.90, 0.05], [0.00, 0.20, 0.80]])
    cmsm = {"transition_matrix": T, "pi": np.array([0.25, 0.5, 0.25]), "active_set": np.array([0, 1, 2])}
    assert least_flux_pair(cmsm) == (1, 0)
    meta = np.array([0, 0, 1, 1, 2, 2, 1])                                   # 7 microstates in 3 sets
    dtraj = np.random.default_rng(1).integers(0, 7, size=500)
    s, e, si, ei = tps_endpoints(cmsm, meta, dtraj, 40, 137, 2)
    assert (s, e) == (1, 0) and si.shape == ei.shape == (40,) and si.dtype == np.int64
    assert (meta[dtraj[si]] == s).all() and (meta[dtraj[ei]] == e).all() and len(set(si.tolist())) > 10
    again = tps_endpoints(cmsm, meta, dtraj, 40, 137, 2)
    assert np.array_equal(again[2], si) and np.array_equal(again[3], ei)
    assert np.array_equal(tps_endpoints(cmsm, meta, dtraj, 10, 137, 2)[2], si[:10])       # path by path, in order
    other = tps_endpoints(cmsm, meta, dtraj, 40, 137, 3)
    assert not np.array_equal(other[2], si) and not np.array_equal(other[3], ei)
    rng = np.random.default_rng([137, 2])                                     # the stated draw order
    starts, ends = np.flatnonzero(meta[dtraj] == 1), np.flatnonzero(meta[dtraj] == 0)
    assert si[0] == starts[rng.integers(len(starts))] and ei[0] == ends[rng.integers(len(ends))]
    with pytest.raises(ValueError, match="no start or end state found"):
        tps_endpoints(cmsm, meta, np.full(100, 2), 4, 137, 0)                # only state 1: the end state 0 has no frame


def test_msm_still_imports_without_torch_or_scipy():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; sys.modules['scipy'] = None; import mdgen_amd.msm as M; import numpy as np; "
            "print(M.bridge_exact(np.full((2, 2), 0.5), 0, 1, 3)['Z'], M.state_probs(np.array([[0, 1]]), 2).tolist())")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "0.5 [0.5, 0.5]", r.stderr


# ---- the command lines -----------------------------------------------------------------------------------------------
def test_tps_inference_parser_keeps_todays_command_lines():
    from mdgen_amd import tps_inference as cli
    p = cli.build_parser()
    a = p.parse_args(["--sim_ckpt", "m.ckpt", "--data_dir", "d", "--num_frames", "100", "--num_batches", "2", "--batch_size", "5",
                      "--out_dir", "o", "--split", "s.csv", "--start_frame", "3", "--end_frame", "77", "--pdb_id", "AAAA", "BBBB"])
    assert (a.sim_ckpt, a.data_dir, a.num_frames, a.num_batches, a.batch_size, a.out_dir, a.split, a.start_frame, a.end_frame,
            a.pdb_id) == ("m.ckpt", "d", 100, 2, 5, "o", "s.csv", 3, 77, ["AAAA", "BBBB"])
    assert not a.msm and not a.npy and not a.synthetic
    d = p.parse_args([])
    assert (d.data_dir, d.suffix, d.num_frames, d.num_batches, d.batch_size, d.out_dir, d.split, d.chunk_idx, d.n_chunks,
            d.start_frame, d.end_frame) == ("share/4AA_data", "", 1000, 100, 10, ".", "splits/4AA_test.csv", 0, 1, 0, -1)
    assert (d.tica_lag, d.msm_k, d.msm_states, d.md_msm_lag, d.kmeans_seed, d.tps_seed) == (1000, 100, 10, 1000, 137, 137)
    m = p.parse_args(["--msm", "--npy", "--msm_k", "12", "--msm_states", "3", "--md_msm_lag", "5", "--tica_lag", "5",
                      "--kmeans_seed", "7", "--tps_seed", "9"])
    assert m.msm and m.npy and (m.tica_lag, m.msm_k, m.msm_states, m.md_msm_lag, m.kmeans_seed, m.tps_seed) == (5, 12, 3, 5, 7, 9)


def _metadata(tmp_path, name="pA", paths=2):
    T = np.array([[0.9, 0.1], [0.2, 0.8]])
    cmsm = {"lag": 1, "active_set": np.array([0, 1]), "count_matrix": np.ones((2, 2), np.int64), "transition_matrix": T,
            "pi": np.array([2 / 3, 1 / 3])}
    with open(tmp_path / f"{name}_metadata.pkl", "wb") as f:
        pickle.dump({"msm": {}, "cmsm": cmsm, "pcca": {}, "kmeans": {}, "tica": {}, "ref_kmeans": np.zeros(3, np.int32)}, f)
    meta = [{"name": name, "start_idx": 0, "end_idx": 1, "start_state": 0, "end_state": 1, "path": f"{name}_{i}.pdb"}
            for i in range(paths)]
    json.dump(meta, open(tmp_path / f"{name}_metadata.json", "w"))


def test_analyze_peptide_tps_named_errors(tmp_path):
    from mdgen_amd import analyze_peptide_tps as cli
    p = cli.build_parser()
    d = p.parse_args(["--pdbdir", "x", "--outdir", "y"])
    assert (d.stride, d.n_samples, d.seed, d.suffix, d.save_name, d.repdir) == (10, 1000, 137, "", "out.pkl", "share/4AA_sims_replica")
    assert d.rep_lens == [999999, 500000, 300000, 200000, 100000, 50000, 20000]
    assert d.rep_names == ["100ns", "50ns", "30ns", "20ns", "10ns", "5ns", "2ns"]
    for gone in ("--plot", "--num_workers", "--mddir"):
        with pytest.raises(SystemExit):
            p.parse_args(["--pdbdir", "x", "--outdir", "y", gone, "1"])
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\npA,FLRH\n")
    common = ["--pdbdir", str(tmp_path), "--outdir", str(tmp_path / "out"), "--split", str(split), "--pdb_id", "pA"]
    with pytest.raises(SystemExit, match="unequal"):
        cli.main(common + ["--rep_lens", "100", "50", "--rep_names", "a"])
    with pytest.raises(SystemExit, match="pA_metadata.json"):                  # missing metadata, before a device is touched
        cli.main(common)
    _metadata(tmp_path)
    os.remove(tmp_path / "pA_metadata.pkl")
    with pytest.raises(SystemExit, match="pA_metadata.pkl"):
        cli.main(common)
    _metadata(tmp_path)
    with pytest.raises(SystemExit, match="neither .*pA_0.npy nor .pdb"):       # a listed path is missing
        cli.main(common)
    np.save(tmp_path / "pA_0.npy", np.zeros((12, 4, 14, 3), np.float32))
    np.save(tmp_path / "pA_1.npy", np.zeros((11, 4, 14, 3), np.float32))
    with pytest.raises(SystemExit, match="ragged.*pA_1.*11 frames.*12"):
        cli.main(common)
