"""csrc/k_analysis.hip on the GPU against tests/analysis_ref.py (gates: its docstring).

Every output buffer is pre-filled with a sentinel and has a guard region of the sentinel behind it; the guards must be intact and
no sentinel may be left where an output belongs.  Histograms are compared with np.histogram / np.histogram2d of the angles copied
back from the device, exactly."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
SENT_F = -7777.0
SENT_I = -(1 << 40)


def _cuda():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _guarded(n, dtype, sentinel):
    buf = torch.full((n + GUARD,), sentinel, dtype=dtype, device=_cuda())
    return buf, buf[:n]


def _guard_ok(buf, n, sentinel):
    assert (buf[n:] == sentinel).all().item(), "guard overwritten"


# ---- dihedrals ------------------------------------------------------------------------------------------------------
def run_dihedrals(atom14, quad):
    from mdgen_amd.analysis import dihedrals_into
    F, NF = atom14.shape[0], len(quad)
    buf, out = _guarded(F * NF, torch.float32, SENT_F)
    dihedrals_into(torch.from_numpy(np.array(atom14, np.float32)).to(_cuda()), quad, out)   # (a copy: the cases are read-only)
    torch.cuda.synchronize()
    _guard_ok(buf, F * NF, SENT_F)
    got = out.cpu().numpy().reshape(F, NF)
    assert not (got == SENT_F).any(), "an angle was not written"
    return got


def check_dihedrals(F, seq, seed=11):
    a, aatype, labels, quad, ref, well, gate = R.dihedral_case(F, tuple(int(x) for x in seq), seed)
    got = run_dihedrals(a, quad)
    assert np.isfinite(got).all() and (np.abs(got) <= float(R.PI32)).all()
    if well.any():
        err = R.wrapped(got, ref)[well].max()
        print(f"dihedrals F {F} L {len(aatype)} NF {len(labels)}: error {err:.3e}, gate {gate:.3e}")
        assert err <= gate, (err, gate)


@pytest.mark.parametrize("L", [1, 2, 4, 33])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 257, 4099])
def test_dihedrals_frame_counts_and_lengths(F, L):
    check_dihedrals(F, R.grid_sequence(L))


def test_dihedrals_every_residue_type_and_length():
    for a in range(20):                                      # L = 1: chi angles only; GLY and ALA: NF = 0, nothing written
        check_dihedrals(65, [a])
    for i in range(0, 20, 2):                                # L = 2
        check_dihedrals(65, [i, i + 1])
    for seq in R.ALL_TYPES_4:                                # L = 4
        check_dihedrals(65, R.aatype_of(seq))
    check_dihedrals(65, R.mixed_types(33))                   # L = 33: 128 features, two launches of 64 quadruples


def test_dihedrals_degenerate_and_trans():
    quad = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [0, 0, 1, 2], [4, 5, 6, 7]], np.int32)
    a = np.zeros((3, 1, 14, 3), np.float32)
    a[1, 0, :4] = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]          # collinear; atoms 4 .. 7 coincide at the origin
    a[2, 0, :4] = [[0, 1, 0], [0, 0, 0], [1.5, 0, 0], [1.5, -1, 0]]     # planar trans
    a[2, 0, 4:8] = [[3, 1, -2], [3, 0, -2], [4.5, 0, -2], [4.5, -1, -2]]
    got = run_dihedrals(a, quad)
    assert np.array_equal(got[0], np.zeros(4, np.float32)) and np.array_equal(got[1], np.zeros(4, np.float32))
    assert not np.signbit(got[:2]).any()
    gate = max(32 * float(R.wrapped(R.dihedrals_torch32(a[2:], quad[[0, 1, 3]]), np.pi).max()), R.EPS32)
    assert (np.abs(np.abs(got[2, [0, 1, 3]]) - np.pi) <= gate).all(), got[2]   # either sign of pi
    assert got[2, 2] == 0                                                      # a repeated atom: b1 = 0


def test_dihedral_refusal_leaves_the_output_alone():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.analysis import dihedrals_into
    buf, out = _guarded(8, torch.float32, SENT_F)
    a = torch.zeros(4, 1, 14, 3, device=_cuda())
    with pytest.raises(MdgenError, match="outside the frame"):
        dihedrals_into(a, np.array([[0, 1, 2, 3], [0, 1, 2, 14]], np.int32), out)
    torch.cuda.synchronize()
    assert (buf == SENT_F).all().item()


# ---- histograms -----------------------------------------------------------------------------------------------------
def run_histograms(angles, pairs, bins1=R.BINS_1D, bins2=R.BINS_2D):
    from mdgen_amd.analysis import hist_edges, histograms_into
    dev = _cuda()
    ang = angles if torch.is_tensor(angles) else torch.from_numpy(np.ascontiguousarray(angles, np.float32)).to(dev)
    F, NF = ang.shape
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    n1, n2, n3 = NF * bins1, P * bins2 * bins2, NF + P
    b1, h1 = _guarded(n1, torch.int64, SENT_I)
    b2, h2 = _guarded(n2, torch.int64, SENT_I)
    b3, dr = _guarded(n3, torch.int64, SENT_I)
    histograms_into(ang, pairs, bins1, torch.from_numpy(hist_edges(bins1)).to(dev), bins2, torch.from_numpy(hist_edges(bins2)).to(dev),
                    h1, h2, dr)
    torch.cuda.synchronize()
    for b, n in ((b1, n1), (b2, n2), (b3, n3)):
        _guard_ok(b, n, SENT_I)
    return h1.cpu().numpy().reshape(NF, bins1), h2.cpu().numpy().reshape(P, bins2, bins2), dr.cpu().numpy()


def check_histograms(angles, pairs):
    back = angles.cpu().numpy() if torch.is_tensor(angles) else np.asarray(angles, np.float32)
    got = run_histograms(angles, pairs)
    want = R.numpy_histograms(back, pairs)
    for g, w, what in zip(got, want, ("hist1", "hist2", "dropped")):
        assert np.array_equal(g, w), what
    F, NF = back.shape
    assert (got[0].sum(1) + got[2][:NF] == F).all() and (got[1].sum((1, 2)) + got[2][NF:] == F).all()
    return got


@pytest.mark.parametrize("NF", [1, 23])
@pytest.mark.parametrize("F", [1, 1000, 100003])
def test_histograms_of_device_angles(F, NF):
    """Angles the dihedral kernel produced (L = 1 TRP / a 7-residue sequence with 23 torsions), binned where they are."""
    from mdgen_amd.analysis import torsion_features
    aatype = R.aatype_of("W") if NF == 1 else R.aatype_of("FLRHAGS")
    labels, quad = torsion_features(aatype)
    quad = quad[:NF]
    assert len(quad) == NF
    g = np.random.default_rng(F + NF)
    a = torch.from_numpy((g.normal(size=(F, len(aatype), 14, 3)) * 3).astype(np.float32)).to(_cuda())
    from mdgen_amd.analysis import dihedrals_into
    ang = torch.empty(F, NF, dtype=torch.float32, device=_cuda())
    dihedrals_into(a, quad, ang)
    check_histograms(ang, [(0, 0)] if NF == 1 else [(1, 2), (3, 4), (22, 0)])


def test_histograms_at_the_edges():
    e = R.edge_angles()
    h1, h2, dr = check_histograms(e, [(0, 1), (1, 0)])
    outside = (e[:, 0].astype(np.float64) > np.pi).sum() + (e[:, 0].astype(np.float64) < -np.pi).sum()
    assert dr[0] == outside >= 4 and float(R.PI32) > np.pi
    only_pi = np.full((5, 1), R.PI32, np.float32)
    h1, _, dr = check_histograms(only_pi, [])
    assert h1.sum() == 0 and dr[0] == 5                      # float32(pi) > np.pi: dropped, as np.histogram drops it
    h1, _, dr = check_histograms(np.full((5, 1), np.float32(np.nextafter(R.PI32, np.float32(0))), np.float32), [])
    assert h1[0, 99] == 5 and dr[0] == 0


def test_histograms_with_more_pairs_than_a_launch_takes():
    ang = R.random_angles(1000, 5, seed=2)
    pairs = [(i % 5, (i * 3 + 1) % 5) for i in range(70)]    # 64 pairs a launch
    check_histograms(ang, pairs)
    got = run_histograms(ang, [(0, 1)], bins1=7, bins2=3)
    want = R.numpy_histograms(ang, [(0, 1)], bins1=7, bins2=3)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- autocovariance -------------------------------------------------------------------------------------------------
def run_acov(angles, K):
    from mdgen_amd.analysis import acov_into, acov_workspace_bytes
    dev = _cuda()
    n, NF = angles.shape
    ws = torch.empty(acov_workspace_bytes(n, NF, K), dtype=torch.uint8, device=dev)
    na = NF * (K + 1)
    ba, acov = _guarded(na, torch.float64, SENT_F)
    bs, ms = _guarded(NF, torch.float64, SENT_F)
    bc, mc = _guarded(NF, torch.float64, SENT_F)
    acov_into(torch.from_numpy(np.ascontiguousarray(angles, np.float32)).to(dev), K, acov, ms, mc, ws)
    torch.cuda.synchronize()
    for b, m in ((ba, na), (bs, NF), (bc, NF)):
        _guard_ok(b, m, SENT_F)
    out = acov.cpu().numpy().reshape(NF, K + 1), ms.cpu().numpy(), mc.cpu().numpy()
    assert not any((o == SENT_F).any() for o in out), "an output was not written"
    return out


ACOV_CASES = [(1, 0, 1), (1, 0, 23), (2, 1, 1), (2, 1, 23), (65, 64, 1), (65, 64, 23), (1001, 1000, 1), (1001, 1000, 23),
              (4097, 1000, 1), (4097, 1000, 23), (100003, 1000, 4)]


@pytest.mark.parametrize("n,K,NF", ACOV_CASES)
def test_acov(n, K, NF):
    ang = R.random_angles(n, NF, seed=n + NF)
    got, ms, mc = run_acov(ang, K)
    want, wms, wmc = R.acov_fft(ang, K)
    lags = None if n * NF <= 5000 else sorted(set(range(0, K + 1, 37)) | {1, K - 1, K})   # (the floor: np.dot per lag and feature)
    gate = R.acov_gate(ang, K, lags)
    err = np.abs(got - want).max()
    print(f"acov n {n} K {K} NF {NF}: error {err:.3e}, gate {gate:.3e}")
    assert err <= gate, (err, gate)
    assert np.abs(got[:, 0] - 1).max() <= gate
    assert max(np.abs(ms - wms).max(), np.abs(mc - wmc).max()) <= gate
    again = run_acov(ang, K)
    assert all(np.array_equal(a, b) for a, b in zip((got, ms, mc), again)), "a second call gave other bits"


def test_acov_of_a_constant_series():
    from mdgen_amd.analysis import decorrelation
    for value in (0.7, 0.0):
        ang = np.full((4097, 2), value, np.float32)
        got, ms, mc = run_acov(ang, 1000)
        gate = R.acov_gate(ang, 1000, range(0, 1001, 100))
        assert np.abs(got - 1).max() <= gate, (value, np.abs(got - 1).max(), gate)
    # baseline exactly 1 at angle 0 (sin 0, cos 1: what a degenerate quadruple gives): 0 / 0
    d = decorrelation(torch.zeros(4097, 2, device=_cuda()), 1000)
    assert d.shape == (2, 1001) and torch.isnan(d).all().item()


def test_acov_refuses_K_equal_n():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.analysis import acov_into
    dev = _cuda()
    ba, acov = _guarded(2 * 66, torch.float64, SENT_F)
    bm, ms = _guarded(4, torch.float64, SENT_F)
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=dev)
    with pytest.raises(MdgenError, match="K must be in 0 .. n - 1"):
        acov_into(torch.zeros(65, 2, device=dev), 65, acov, ms[:2], ms[2:], ws)
    torch.cuda.synchronize()
    assert (ba == SENT_F).all().item() and (bm == SENT_F).all().item() and (ws == 0x5A).all().item()


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_analyze_against_the_restatement():
    from mdgen_amd.analysis import analyze, featurize
    dev = _cuda()
    aatype = R.aatype_of("FLRH")
    traj, ref = R.peptide(2000, aatype, seed=21, walk=0.15), R.peptide(5000, aatype, seed=22, walk=0.15)
    got = analyze(torch.from_numpy(traj).to(dev), ref, aatype, nlag=200, ref_nlag=200)
    a_traj = featurize(torch.from_numpy(traj).to(dev), aatype).cpu().numpy()
    a_ref = featurize(torch.from_numpy(ref).to(dev), aatype).cpu().numpy()
    want = R.analyze(traj, ref, aatype, nlag=200, ref_nlag=200, angles=(a_traj, a_ref))   # (the device's angles: exact counts)
    assert got["features"] == want["features"] and list(got["JSD"]) == list(want["JSD"]) and len(got["JSD"]) == 16 + 2
    assert list(got) == ["features", "JSD", "our_decorrelation", "md_decorrelation"]
    for k, v in want["JSD"].items():
        assert abs(got["JSD"][k] - v) <= 1e-12, k
        assert isinstance(got["JSD"][k], float) and 0 < v < 0.84
    for key, ang in (("our_decorrelation", a_traj), ("md_decorrelation", a_ref)):
        gate = R.acov_gate(ang, 200, range(0, 201, 20))
        _, ms, mc = R.acov_fft(ang, 200)
        base = ms * ms + mc * mc
        for i, lab in enumerate(got["features"]):
            g, w = got[key][lab], want[key][lab]
            assert g.dtype == np.float32 and g.shape == (201,)
            tol = gate / (1 - base[i])
            assert np.abs(g.astype(np.float64) - w).max() <= tol, (key, lab)


def test_sim_inference_analyze(tmp_path):
    """sim_inference --synthetic --analyze --npy, 2 peptides: analysis.pkl holds analyze() of each .npy; without the flag, no file."""
    from oracle import mdgen_oracle as O
    from mdgen_amd import sim_inference as cli
    from mdgen_amd.analysis import analyze
    from mdgen_amd.geometry import restype_order
    dev = _cuda()
    names = {"FLRH": "FLRH", "AWKD": "AWKD"}
    gen = torch.Generator().manual_seed(5)
    data = tmp_path / "data"
    data.mkdir()
    for n, sq in names.items():
        seqres = torch.tensor([restype_order[ch] for ch in sq])
        q = torch.randn(1, 3, 4, 4, generator=gen)
        tr = torch.cumsum(2.2 * torch.randn(1, 3, 4, 3, generator=gen), 2)
        ang = torch.randn(1, 3, 4, 7, 2, generator=gen)
        arr = O.frames_torsions_to_atom14(O.quat_to_rot(q / q.norm(dim=-1, keepdim=True)), tr, ang / ang.norm(dim=-1, keepdim=True),
                                          seqres[None, None].expand(1, 3, 4))[0].numpy().astype(np.float16)
        np.save(data / f"{n}.npy", arr)
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\n" + "".join(f"{n},{s}\n" for n, s in names.items()))
    common = ["--synthetic", "--data_dir", str(data), "--split", str(split), "--num_frames", "50", "--num_rollouts", "2",
              "--num_steps", "2", "--batch", "2", "--npy"]
    out = tmp_path / "out"
    res = cli.main(common + ["--out_dir", str(out), "--analyze"])
    assert res["names"] == list(names) and res["frames"] == 2 * 2 * 50
    got = pickle.load(open(out / "analysis.pkl", "rb"))
    assert list(got) == list(names)
    for n, sq in names.items():
        aat = np.array([restype_order[c] for c in sq])
        want = analyze(torch.from_numpy(np.load(out / f"{n}.npy")).to(dev), np.load(data / f"{n}.npy"), aat)
        assert got[n]["features"] == want["features"] and got[n]["JSD"].keys() == want["JSD"].keys()
        for k in want["JSD"]:
            assert got[n]["JSD"][k] == want["JSD"][k] or (np.isnan(got[n]["JSD"][k]) and np.isnan(want["JSD"][k]))
        for key in ("our_decorrelation", "md_decorrelation"):
            for lab in want["features"]:
                assert np.array_equal(got[n][key][lab], want[key][lab], equal_nan=True), (n, key, lab)
        assert got[n]["our_decorrelation"][want["features"][0]].shape == (100,)   # nlag clamped to 2 * 50 - 1
    out2 = tmp_path / "out2"
    cli.main(common + ["--out_dir", str(out2)])
    assert (out2 / "FLRH.pdb").exists() and not (out2 / "analysis.pkl").exists()


def test_cli_analyze_peptide_sim(tmp_path):
    """analyze_peptide_sim --no_msm --save: one peptide read from its .npy, one from its multi-model PDB (no .npy beside it);
    the pickle holds analyze() of what was read."""
    from mdgen_amd import analyze_peptide_sim as cli
    from mdgen_amd.analysis import analyze
    from mdgen_amd.pdb import atom14_to_pdb, pdb_to_atom14
    dev = _cuda()
    names = {"pA": "FLRH", "pB": "AWKD"}
    out, data = tmp_path / "out", tmp_path / "data"
    out.mkdir()
    data.mkdir()
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\n" + "".join(f"{n},{s}\n" for n, s in names.items()) + "pC,GGGG\n")   # pC: no trajectory
    trajs = {}
    for i, (n, sq) in enumerate(names.items()):
        aat = R.aatype_of(sq)
        trajs[n] = R.peptide(300, aat, seed=30 + i, walk=0.2)
        np.save(data / f"{n}.npy", R.peptide(400, aat, seed=40 + i, walk=0.2).astype(np.float16))
    np.save(out / "pA.npy", trajs["pA"])
    atom14_to_pdb(trajs["pB"], R.aatype_of("AWKD"), str(out / "pB.pdb"))
    got = cli.main(["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--no_msm", "--no_traj_msm", "--save",
                    "--truncate", "250"])
    saved = pickle.load(open(out / "out.pkl", "rb"))
    assert list(got) == list(saved) == ["pA", "pB"]
    read = {"pA": trajs["pA"], "pB": pdb_to_atom14(str(out / "pB.pdb"), R.aatype_of("AWKD"))}
    assert not np.array_equal(read["pB"], trajs["pB"]) and np.abs(read["pB"] - trajs["pB"]).max() <= 5.1e-4   # three decimals
    for n, sq in names.items():
        want = analyze(torch.from_numpy(read[n][:250]).to(dev), np.load(data / f"{n}.npy"), R.aatype_of(sq))
        assert saved[n]["features"] == want["features"] and saved[n]["JSD"] == want["JSD"]
        for key in ("our_decorrelation", "md_decorrelation"):
            assert all(np.array_equal(saved[n][key][lab], want[key][lab], equal_nan=True) for lab in want["features"])
        assert saved[n]["our_decorrelation"][want["features"][0]].shape == (250,)
        assert saved[n]["md_decorrelation"][want["features"][0]].shape == (400,)
    short = cli.main(["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--no_msm", "--no_decorr", "--pdb_id", "pA"])
    assert list(short) == ["pA"] and list(short["pA"]) == ["features", "JSD"]
