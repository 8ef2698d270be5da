"""mdgen_amd.analysis without a device: the entry points' bindings and refusals, the feature table, the host functions, the PDB
reader, the command line's refusals -- and tests/analysis_ref.py, the NumPy restatement the kernels are held against on the GPU,
against independent evaluations (np.histogram, a double loop, scipy, hand-built geometry)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mdgen_traj_dihedrals": ["F", "L", "NF", "atom14", "quad", "angles", "stream"],
       "mdgen_traj_histograms": ["F", "NF", "angles", "bins1", "edges1", "P", "pairs", "bins2", "edges2", "hist1", "hist2",
                                 "dropped", "stream"],
       "mdgen_traj_acov_workspace_bytes": ["n", "NF", "K", "bytes"],
       "mdgen_traj_acov": ["n", "NF", "K", "angles", "acov", "mean_sin", "mean_cos", "workspace", "workspace_bytes", "stream"]}


def test_header_exports_and_binding_agree():
    import mdgen_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    kind = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
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
    """Every refusal is decided on the host: the pointers are never dereferenced (the index tables, host arrays, are read)."""
    import mdgen_amd._lib as L
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    quad = np.array([[0, 1, 2, 14]], np.int32)
    pairs = np.array([[0, 1]], np.int32)
    err = L.lib.mdgen_last_error
    dih, hist, acov, wsb = (L.lib.mdgen_traj_dihedrals, L.lib.mdgen_traj_histograms, L.lib.mdgen_traj_acov,
                            L.lib.mdgen_traj_acov_workspace_bytes)
    assert dih(0, 2, 1, p, quad.ctypes.data, p, None) == -2 and b"F" in err()
    assert dih(1, 0, 1, p, quad.ctypes.data, p, None) == -2
    assert dih(1, 1, 1, p, quad.ctypes.data, p, None) == -2 and b"quad[0][3] = 14" in err()        # L = 1: 14 atoms
    assert dih(1, 2, 1, p, np.array([[0, -1, 2, 3]], np.int32).ctypes.data, p, None) == -2
    assert dih(1, 2, 1, None, quad.ctypes.data, p, None) == -1 and b"null" in err()
    assert dih(1, 2, 0, None, None, None, None) == 0                                                # NF = 0: nothing to do
    ok = lambda F=1, NF=2, b1=100, P=1, pr=pairs, b2=50: hist(F, NF, p, b1, p, P, pr.ctypes.data, b2, p, p, p, p, None)  # noqa: E731
    assert ok(F=0) == -2 and ok(b1=0) == -2 and ok(b2=0) == -2 and ok(b2=129) == -2 and ok(b1=16385) == -2
    assert ok(NF=1) == -2 and b"pairs[0][1] = 1" in err()
    assert ok(pr=np.array([[-1, 0]], np.int32)) == -2
    assert hist(1, 2, None, 100, p, 0, None, 50, None, p, None, p, None) == -1
    assert hist(1, 0, None, 100, None, 0, None, 50, None, None, None, None, None) == 0
    for n, K in ((0, 0), (5, 5), (5, -1), (1, 1)):
        assert acov(n, 1, K, p, p, p, p, p, 1 << 20, None) == -2, (n, K)
        assert b"must be in" in err()
    assert acov(5, 1, 4, p, p, p, p, p, 0, None) == -3
    assert acov(5, 1, 4, p, None, p, p, p, 1 << 20, None) == -1
    assert acov(5, 0, 4, None, None, None, None, None, 0, None) == 0
    b = ctypes.c_size_t()
    assert wsb(5, 1, 5, ctypes.byref(b)) == -2 and wsb(5, 1, 4, None) == -1
    # the sampler's size and the reference's MD size fit a launch and a device: 25 features, (1e5, 1e3) and (1e6, 1e5)
    assert wsb(100000, 25, 1000, ctypes.byref(b)) == 0 and 2 * 25 * 100000 * 4 <= b.value < 1 << 28
    assert wsb(1000000, 25, 100000, ctypes.byref(b)) == 0 and b.value < 1 << 30


def test_torsion_features_cover_every_residue_type():
    from mdgen_amd.analysis import torsion_features
    from mdgen_amd.pdb import residue_tables
    t = residue_tables()
    seen = set()
    for seq in R.ALL_TYPES_4:
        aatype = R.aatype_of(seq)
        seen |= set(aatype.tolist())
        labels, quad = torsion_features(aatype)
        n_chi = [int(sum(t["chi_angles_mask"][a][c] for a in aatype)) for c in range(4)]
        assert quad.shape == (6 + sum(n_chi), 4) and quad.dtype == np.int32 and len(labels) == len(quad)
        kinds = [lab.split()[0] for lab in labels]
        assert kinds == ["PHI"] * 3 + ["PSI"] * 3 + sum((["CHI%d" % (c + 1)] * n_chi[c] for c in range(4)), [])
        assert [int(lab.split()[3]) for lab in labels[:6]] == [1, 2, 3, 0, 1, 2]
        for lab in labels:
            k, chain, r3, num = lab.split()
            assert chain == "0" and r3 == str(t["restype_3"][aatype[int(num)]])
            if k.startswith("CHI"):
                assert t["chi_angles_mask"][aatype[int(num)]][int(k[3]) - 1] == 1
        for i, a in enumerate(aatype):   # per residue, the chi count of its type
            assert sum(lab.startswith("CHI") and int(lab.split()[3]) == i for lab in labels) == int(t["chi_angles_mask"][a].sum())
        present = t["atom14_mask"][aatype].reshape(-1)
        assert (present[quad] == 1).all(), "a quadruple names an atom its residue does not have"
        bb, _ = torsion_features(aatype, sidechains=False)
        assert bb == labels[:6]
    assert seen == set(range(20))
    assert torsion_features(R.aatype_of("ALKA"))[0][:7] == ["PHI 0 LEU 1", "PHI 0 LYS 2", "PHI 0 ALA 3", "PSI 0 ALA 0", "PSI 0 LEU 1",
                                                          "PSI 0 LYS 2", "CHI1 0 LEU 1"]
    # phi = C(i-1) N CA C, psi = N CA C N(i+1) in atom14 slots (N 0, CA 1, C 2)
    _, q = torsion_features(R.aatype_of("GG"))
    assert q.tolist() == [[2, 14, 15, 16], [0, 1, 2, 14]]


def test_torsion_features_of_one_residue():
    from mdgen_amd.analysis import torsion_features
    from mdgen_amd.pdb import residue_tables
    t = residue_tables()
    for a in range(20):
        labels, quad = torsion_features(np.array([a]))
        n = int(t["chi_angles_mask"][a].sum())
        assert len(labels) == n and quad.shape == (n, 4) and all(lab.startswith("CHI") for lab in labels)
    assert torsion_features(R.aatype_of("G"))[0] == [] and torsion_features(R.aatype_of("A"))[0] == []
    assert torsion_features(R.aatype_of("R"))[0] == ["CHI%d 0 ARG 0" % c for c in (1, 2, 3, 4)]   # (no chi5)


def _four(angle_deg):
    """Four atoms with p0 along +x from p1, the bond p1-p2 along +z, p3 turned by the angle about it."""
    th = np.deg2rad(angle_deg)
    return np.array([[1.0, 0, 0], [0, 0, 0], [0, 0, 1.5], [np.cos(th), np.sin(th), 1.5]])


def test_reference_dihedrals_on_hand_built_geometry():
    quad = np.array([[0, 1, 2, 3]])
    for deg in (0.0, 90.0, -90.0, 180.0, 37.5, -120.0):
        a = np.zeros((1, 1, 14, 3))
        a[0, 0, :4] = _four(deg)
        got = R.dihedrals(a, quad)[0, 0]
        assert R.wrapped(got, np.deg2rad(deg)) < 1e-15, (deg, got)
    # a known phi / psi: an alpha-helical pair built from internal coordinates (phi -57, psi -47)
    def place(a, b, c, bond, angle, tors):   # noqa: E306  (NeRF: the atom at `bond` from c, `angle` at c, torsion a-b-c-d)
        bc = (c - b) / np.linalg.norm(c - b)
        n = np.cross(b - a, bc)
        n /= np.linalg.norm(n)
        m = np.cross(n, bc)
        d = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(tors), bond * np.sin(angle) * np.sin(tors)])
        return c + d[0] * bc + d[1] * m + d[2] * n
    phi, psi, om = np.deg2rad(-57.0), np.deg2rad(-47.0), np.pi
    c0, n1, ca1 = np.array([0.0, 1.3, 0.2]), np.array([1.2, 0.9, 0.0]), np.array([2.2, 1.9, 0.4])
    c1 = place(c0, n1, ca1, 1.52, np.deg2rad(111.0), phi)
    n2 = place(n1, ca1, c1, 1.33, np.deg2rad(116.0), psi)
    ca2 = place(ca1, c1, n2, 1.46, np.deg2rad(122.0), om)
    a = np.zeros((1, 3, 14, 3))
    a[0, 0, 2], a[0, 1, 0], a[0, 1, 1], a[0, 1, 2], a[0, 2, 0], a[0, 2, 1] = c0, n1, ca1, c1, n2, ca2
    from mdgen_amd.analysis import torsion_features
    labels, q = torsion_features(R.aatype_of("GGG"))
    got = R.dihedrals(a, q)[0]
    assert labels[1] == "PHI 0 GLY 2" and labels[2] == "PSI 0 GLY 0"
    assert R.wrapped(got[0], phi) < 1e-12 and R.wrapped(got[3], psi) < 1e-12   # phi and psi of residue 1
    assert np.array_equal(R.dihedrals(np.zeros((2, 3, 14, 3)), q), np.zeros((2, 4)))   # coincident atoms: atan2(0, 0) = 0


def test_dihedral_cases_are_well_conditioned():
    """The cap of the GPU test's gate: at most 1 % of a case's quadruples may be ill-conditioned (asserted in dihedral_case)."""
    for seq in R.ALL_TYPES_4:
        a, aatype, labels, quad, ref, well, gate = R.dihedral_case(65, tuple(R.aatype_of(seq)), 11)
        assert a.shape == (65, 4, 14, 3) and a.dtype == np.float32 and ref.shape == (65, len(labels))
        assert R.EPS32 <= gate < 1e-3
    assert R.dihedral_case(65, tuple(R.mixed_types(33)), 11)[4].shape[1] > 100
    for F in R.DIHEDRAL_F:                     # the grid the GPU test runs
        for L_ in R.DIHEDRAL_L:
            a, aatype, labels, quad, ref, well, gate = R.dihedral_case(F, tuple(int(x) for x in R.grid_sequence(L_)), 11)
            assert ref.shape == (F, len(labels)) and len(labels) >= 4 and R.EPS32 <= gate < 2e-3, (F, L_, gate)


def test_jsd_equals_scipy():
    sp = pytest.importorskip("scipy.spatial.distance")
    from mdgen_amd.analysis import jsd
    g = np.random.default_rng(0)
    for n in (2, 100, 2500):
        p, q = g.integers(0, 50, n), g.integers(0, 50, n)
        p[::3] = 0
        q[1::4] = 0
        assert abs(jsd(p, q) - sp.jensenshannon(p, q)) < 1e-14
        assert jsd(p, p) == 0.0
    p, q = np.array([3, 1, 0, 0]), np.array([0, 0, 2, 5])
    assert abs(jsd(p, q) - np.sqrt(np.log(2))) < 1e-15 and abs(sp.jensenshannon(p, q) - np.sqrt(np.log(2))) < 1e-15
    assert np.isnan(jsd(np.zeros(4), q)) and np.isnan(sp.jensenshannon(np.zeros(4), q))


def test_jsd_without_scipy():
    from mdgen_amd.analysis import jsd
    assert jsd([1, 2, 3], [2, 4, 6]) == 0.0 and abs(jsd([1, 0], [0, 1]) - np.sqrt(np.log(2))) < 1e-15
    assert abs(jsd([1, 1], [1, 0]) - np.sqrt((0.5 * np.log(2 / 3) + 0.5 * np.log(2) + np.log(4 / 3)) / 2)) < 1e-15


def test_acov_restatement_equals_the_double_loop():
    ang = R.random_angles(7, 3, seed=3)
    got, ms, mc = R.acov_fft(ang, 6)
    assert np.abs(got - R.acov_direct(ang, 6)).max() < 1e-14
    assert np.abs(got[:, 0] - 1).max() < 1e-14
    assert np.allclose(ms, np.sin(ang.astype(np.float64)).mean(0), atol=1e-16)
    const = np.full((9, 1), 0.7, np.float32)
    assert np.abs(R.acov_fft(const, 8)[0] - 1).max() < 1e-14
    # baseline 1: 0 / 0 where the sums are exact -- direct evaluation at angle 0, which is what a degenerate quadruple gives; at any
    # other constant, or through an FFT, the expression (the reference's) is a ratio of two rounding errors
    with np.errstate(invalid="ignore"):
        assert np.isnan((R.acov_direct(np.zeros((9, 1)), 8) - 1.0) / (1.0 - 1.0)).all()
    assert not np.isfinite(R.decorrelation(np.zeros((9, 1), np.float32), 8)[0, 1:]).any()


def test_histogram_restatement_equals_numpy():
    e = R.edge_angles()
    assert e.dtype == np.float32 and (e[:, 0] == R.PI32).sum() >= 1 and float(R.PI32) > np.pi
    for ang, pairs in ((e, [(0, 1), (1, 0)]), (R.random_angles(1000, 5, seed=1), [(1, 2), (3, 4)])):
        got, want = R.histograms(ang, pairs), R.numpy_histograms(ang, pairs)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert (got[0].sum(1) + got[2][:ang.shape[1]] == len(ang)).all()
    h1, _, dr = R.histograms(e)
    # float32(pi) (twice: as itself and as float32 of the last edge) and its upper neighbour fall outside, and so below -pi
    assert dr[0] == (e[:, 0].astype(np.float64) > np.pi).sum() + (e[:, 0].astype(np.float64) < -np.pi).sum() >= 4
    assert R.bins_of(np.pi, R.hist_edges(100)) == 99 and R.bins_of(-np.pi, R.hist_edges(100)) == 0
    assert R.bins_of(float(R.PI32), R.hist_edges(100)) == -1 and R.bins_of(np.nan, R.hist_edges(100)) == -1


def test_pdb_to_atom14_inverts_the_writer(tmp_path):
    from mdgen_amd.pdb import frames_to_pdb_string, pdb_to_atom14, residue_tables
    aatype = R.aatype_of("SWGR")
    a = R.peptide(5, aatype, seed=2)
    a[2, 1, 5] = 0           # an atom of TRP absent in one frame
    a[3] = 0                 # a frame without atoms
    a[4, 3, 1, 0] = -0.0004  # prints as -0.000
    p = tmp_path / "x.pdb"
    p.write_text(frames_to_pdb_string(a, aatype))
    got = pdb_to_atom14(str(p), aatype)
    mask = residue_tables()["atom14_mask"][aatype][None, :, :, None]
    want = (np.round(a.astype(np.float64) * 1000) / 1000 * mask).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == a.shape
    assert np.array_equal(got, want)
    assert (got[2, 1, 5] == 0).all() and (got[3] == 0).all()
    with pytest.raises(ValueError):
        pdb_to_atom14(str(p), R.aatype_of("SWG"))     # residue 3 of a three-residue sequence
    with pytest.raises(ValueError):
        pdb_to_atom14(str(p), R.aatype_of("SGGR"))    # TRP's atoms on a GLY


def test_cli_refusals(tmp_path, capsys):
    from mdgen_amd import analyze_peptide_sim as cli
    nowhere = str(tmp_path / "nowhere")
    with pytest.raises(SystemExit) as e:   # before anything is read: none of these paths exists
        cli.main(["--pdbdir", nowhere, "--data_dir", nowhere, "--split", nowhere + ".csv"])
    assert e.value.code == 2 and "pyemma" in capsys.readouterr().err
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\npA,FLRH\n")
    (tmp_path / "out").mkdir()
    with pytest.raises(SystemExit) as e:
        cli.main(["--no_msm", "--pdbdir", str(tmp_path / "out"), "--data_dir", nowhere, "--split", str(split), "--pdb_id", "pA"])
    assert "pA" in str(e.value.code) and ".npy" in str(e.value.code)
    np.save(tmp_path / "out" / "pA.npy", np.zeros((2, 4, 14, 3), np.float32))
    with pytest.raises(SystemExit) as e:
        cli.main(["--no_msm", "--pdbdir", str(tmp_path / "out"), "--data_dir", nowhere, "--split", str(split)])
    assert "MD trajectory of pA" in str(e.value.code)


def test_analyze_restatement_keys_and_shapes():
    aatype = R.aatype_of("FLRH")
    traj, ref = R.peptide(50, aatype, seed=4, walk=0.2), R.peptide(80, aatype, seed=5, walk=0.2)
    out = R.analyze(traj, ref, aatype, nlag=1000)
    labels = out["features"]
    assert len(labels) == 3 + 3 + 4 + 4 + 1 + 1   # chi: F 2, L 2, R 4, H 2
    assert list(out) == ["features", "JSD", "our_decorrelation", "md_decorrelation"]
    assert list(out["JSD"]) == labels + [labels[1] + "|" + labels[2], labels[3] + "|" + labels[4]]
    assert all(0 <= v <= np.sqrt(np.log(2)) + 1e-12 for v in out["JSD"].values())
    for lab in labels:
        assert out["our_decorrelation"][lab].shape == (50,) and out["our_decorrelation"][lab].dtype == np.float32   # nlag clamped
        assert out["md_decorrelation"][lab].shape == (80,)
        assert abs(out["our_decorrelation"][lab][0] - 1) < 1e-6
    assert "our_decorrelation" not in R.analyze(traj, ref, aatype, decorr=False)
    short = R.analyze(R.peptide(9, R.aatype_of("GG"), seed=6), R.peptide(9, R.aatype_of("GG"), seed=7), R.aatype_of("GG"))
    assert len(short["features"]) == 2 and list(short["JSD"]) == short["features"]   # two features: neither default pair exists
