"""csrc/k_ensemble.hip and the chain around it on the GPU against tests/ensemble_ref.py (gates: its docstring).

Every output buffer is pre-filled with a sentinel and has a guard region of the sentinel behind it; the guards must be intact, no
sentinel may be left where an output belongs, and a second call gives the same bits."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _written(t, sentinel):
    assert not (t == sentinel).any().item(), "an output was not written"


# ---- superposition ---------------------------------------------------------------------------------------------------
def run_superpose(x, ref, w, exists, in_place=False, with_extras=True):
    from mdgen_amd.ensemble import superpose_into
    F, A = x.shape[:2]
    bo, out = _guarded(F * A * 3, torch.float32, SENT_F)
    br, rot = _guarded(F * 9, torch.float64, SENT_F)
    bm, rmsd = _guarded(F, torch.float64, SENT_F)
    xd = _dev(x)
    if in_place:
        out.copy_(xd.reshape(-1))
        xd = out.reshape(F, A, 3)
    ex = None if exists is None else _dev(exists, np.uint8)
    superpose_into(xd, _dev(ref), _dev(w), ex, out.reshape(F, A, 3), rot if with_extras else None, rmsd if with_extras else None)
    torch.cuda.synchronize()
    _guard_ok(bo, F * A * 3, SENT_F)
    _guard_ok(br, F * 9, SENT_F)
    _guard_ok(bm, F, SENT_F)
    _written(out, SENT_F)
    if with_extras:
        _written(rot, SENT_F)
        _written(rmsd, SENT_F)
    else:
        assert (br == SENT_F).all().item() and (bm == SENT_F).all().item()
    return out.cpu().numpy().reshape(F, A, 3), rot.cpu().numpy().reshape(F, 3, 3), rmsd.cpu().numpy()


@pytest.mark.parametrize("case", R.SUPERPOSE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_superpose(case):
    x, ref, w, exists = R.superpose_case(*case)
    k = R.kabsch(x, ref, w)
    out, rot, rmsd = run_superpose(x, ref, w, exists)
    gate_r = R.rotation_gate(k)
    err_r = np.abs(rot - k["R"]).reshape(len(x), -1).max(1)
    print(f"  rotation: worst error / gate {np.max(err_r / gate_r):.3g} (gate up to {gate_r.max():.2e})")
    assert (err_r <= gate_r).all()
    assert np.abs(np.linalg.det(rot) - 1).max() <= 1e-12
    assert np.abs(np.einsum("fij,fkj->fik", rot, rot) - np.eye(3)).max() <= 1e-12
    want = R.superposed(x, k, exists)
    gate_c = R.coordinate_gate(x, k)
    live = np.ones(x.shape[1], bool) if exists is None else exists != 0
    err_c = np.abs(out.astype(np.float64) - want).max(-1)
    print(f"  coordinates: worst error / gate {np.max(err_c[:, live] / gate_c[:, live]):.3g}")
    assert (err_c[:, live] <= gate_c[:, live]).all()
    assert np.array_equal(out[:, ~live].view(np.uint32), x[:, ~live].view(np.uint32)), "a padded row changed"
    zero = k["rmsd"] < 1e-12                                     # the identity frame: x is ref
    assert (np.abs(rmsd[~zero] - k["rmsd"][~zero]) <= 1e-9 * k["rmsd"][~zero]).all()
    assert (np.abs(rmsd[zero]) <= 1e-6 * R.SCALE).all()
    if len(x) > 1:
        assert zero[0] and np.abs(rot[0] - np.eye(3)).max() <= 1e-14
    again = run_superpose(x, ref, w, exists)
    for a, b in zip((out, rot, rmsd), again):
        assert np.array_equal(a, b), "a second call gave other bits"
    assert np.array_equal(run_superpose(x, ref, w, exists, in_place=True)[0], out), "in place differs"
    assert np.array_equal(run_superpose(x, ref, w, exists, with_extras=False)[0], out)


def test_superpose_wrapper_and_weight_refusals():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.ensemble import superpose, superpose_into
    x, ref, w, exists = R.superpose_case(65, 56, "uniform", True)
    k = R.kabsch(x, ref, w)
    xd = _dev(x).reshape(65, 4, 14, 3)
    out, rot, rmsd = superpose(xd, ref, exists=exists, with_rot=True, with_rmsd=True)     # weights default to exists
    assert out.shape == xd.shape and rot.shape == (65, 3, 3) and rmsd.shape == (65,)
    assert np.array_equal(out.cpu().numpy().reshape(65, 56, 3), run_superpose(x, ref, w, exists)[0])
    assert np.abs(rot.cpu().numpy() - k["R"]).max() <= R.rotation_gate(k).max()
    same = superpose(xd, ref, exists=exists, out=xd)
    assert same.data_ptr() == xd.data_ptr() and torch.equal(xd, out)
    buf, o = _guarded(65 * 56 * 3, torch.float32, SENT_F)
    for bad in (np.where(np.arange(56) == 5, -1.0, 1.0), np.where(np.arange(56) == 7, np.nan, 1.0),
                np.where(np.arange(56) == 7, np.inf, 1.0), np.where(np.arange(56) < 2, 1.0, 0.0), np.zeros(56)):
        with pytest.raises(MdgenError, match="weights must be finite|at least 3 atoms"):
            superpose_into(_dev(x), _dev(ref), _dev(bad), None, o.reshape(65, 56, 3))
    torch.cuda.synchronize()
    assert (buf == SENT_F).all().item()


# ---- moments ---------------------------------------------------------------------------------------------------------
def run_moments(x):
    from mdgen_amd.ensemble import moments_into, moments_workspace_bytes
    F, A = x.shape[:2]
    bm, mean = _guarded(A * 3, torch.float64, SENT_F)
    bc, cov = _guarded(A * 9, torch.float64, SENT_F)
    nws = moments_workspace_bytes(F, A)
    ws = torch.full((nws + GUARD,), 0x5A, dtype=torch.uint8, device=_cuda())
    moments_into(_dev(x), mean, cov, ws[:nws])
    torch.cuda.synchronize()
    _guard_ok(bm, A * 3, SENT_F)
    _guard_ok(bc, A * 9, SENT_F)
    assert (ws[nws:] == 0x5A).all().item(), "workspace guard overwritten"
    _written(mean, SENT_F)
    _written(cov, SENT_F)
    return mean.cpu().numpy().reshape(A, 3), cov.cpu().numpy().reshape(A, 3, 3)


@pytest.mark.parametrize("F,A,offset", R.MOMENTS_CASES)
def test_moments(F, A, offset):
    from mdgen_amd.ensemble import rmsf
    x = R.moments_case(F, A, offset)
    mean, cov = run_moments(x)
    want_m, want_c = R.moments(x)
    gm, gc = R.moments_gates(x)
    em, ec = np.abs(mean - want_m), np.abs(cov - want_c)
    print(f"  mean: worst error {em.max():.3g}; cov: worst error {ec.max():.3g} (largest gates {gm.max():.3g}, {gc.max():.3g})")
    assert (em <= gm).all() and (ec <= gc).all()
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    if F == 1:
        assert (cov == 0).all() and np.array_equal(mean, x[0].astype(np.float64))
    m2, c2 = run_moments(x)
    assert np.array_equal(mean, m2) and np.array_equal(cov, c2), "a second call gave other bits"
    assert np.array_equal(rmsf(_dev(x)), np.sqrt(np.maximum(np.trace(cov, axis1=1, axis2=2), 0.0)))


# ---- pairwise --------------------------------------------------------------------------------------------------------
def run_pairwise(xa, xb, with_matrix=True):
    from mdgen_amd.ensemble import pairwise_d2_into, pairwise_workspace_bytes
    a = _dev(xa)
    b = a if xb is None else _dev(xb)                            # None: the same pointer
    Fa, Fb, A = a.shape[0], b.shape[0], a.shape[1]
    bd, d2 = _guarded(Fa * Fb, torch.float32, SENT_F)
    bs, sums = _guarded(2, torch.float64, SENT_F)
    nws = pairwise_workspace_bytes(Fa, Fb, A)
    ws = torch.full((nws + GUARD,), 0x5A, dtype=torch.uint8, device=_cuda())
    pairwise_d2_into(a, b, d2 if with_matrix else None, sums, ws[:nws])
    torch.cuda.synchronize()
    _guard_ok(bs, 2, SENT_F)
    assert (ws[nws:] == 0x5A).all().item(), "workspace guard overwritten"
    _written(sums, SENT_F)
    if with_matrix:
        _guard_ok(bd, Fa * Fb, SENT_F)
    else:
        assert (bd == SENT_F).all().item()
    return d2.cpu().numpy().reshape(Fa, Fb), sums.cpu().numpy()


@pytest.mark.parametrize("Fa,Fb,A", R.PAIRWISE_CASES)
def test_pairwise_d2(Fa, Fb, A):
    from mdgen_amd.ensemble import pairwise_rmsd
    xa, xb = R.pairwise_case(Fa, Fb, A)
    d2, sums = run_pairwise(xa, xb)
    want = R.pairwise_d2(xa, xa if xb is None else xb)
    assert (d2 >= 0).all()
    err, gate = np.abs(d2.astype(np.float64) - want), (3 * A + 2) * R.EPS32 * want
    print(f"  d2: worst error / gate {np.max(err / np.maximum(gate, 1e-300)):.3g}")
    assert (err <= gate).all()
    if xb is None:
        assert (np.diag(d2) == 0).all() and np.array_equal(d2, d2.T)
    own = R.pairwise_sums(d2, A)
    rel = max(1e-12, 4 * d2.size * R.EPS64)
    assert (np.abs(sums - own) <= rel * own).all(), (sums, own)
    d2b, sums_b = run_pairwise(xa, xb)
    assert np.array_equal(d2, d2b) and np.array_equal(sums, sums_b), "a second call gave other bits"
    assert np.array_equal(run_pairwise(xa, xb, with_matrix=False)[1], sums), "the sums depend on the matrix"
    mean, rms, mat = pairwise_rmsd(_dev(xa), None if xb is None else _dev(xb), matrix=True)
    assert mean == sums[0] / d2.size and rms == np.sqrt(sums[1] / d2.size)
    assert np.allclose(mat.cpu().numpy(), np.sqrt(d2 / np.float32(A)), rtol=1e-6, atol=0)


# ---- contacts --------------------------------------------------------------------------------------------------------
def run_contacts(ca, cutoff=R.CUTOFF):
    from mdgen_amd.ensemble import contact_counts_into
    N = ca.shape[1]
    bc, counts = _guarded(N * N, torch.int32, SENT_I)
    contact_counts_into(_dev(ca), cutoff, counts)
    torch.cuda.synchronize()
    _guard_ok(bc, N * N, SENT_I)
    _written(counts, SENT_I)
    return counts.cpu().numpy().reshape(N, N)


@pytest.mark.parametrize("F,N", R.CONTACT_CASES)
def test_contact_counts(F, N):
    from mdgen_amd.ensemble import contact_counts
    ca = R.contact_case(F, N)
    counts = run_contacts(ca)
    yes, und = R.contact_reference(ca)
    print(f"  undecided {int(und.sum())} of {F * N * N}")
    assert und.sum() <= R.UNDECIDED_CAP * F * N * N
    assert (np.abs(counts - yes) <= und).all()
    assert np.array_equal(counts, counts.T) and (np.diag(counts) == F).all()
    assert np.array_equal(run_contacts(ca), counts), "a second call gave other bits"
    assert np.array_equal(contact_counts(_dev(ca)), counts)
    assert (run_contacts(ca, 1e3) == F).all() and np.array_equal(run_contacts(ca, 0.0), np.zeros((N, N), np.int32))


def test_refusals_leave_the_outputs_alone():
    from mdgen_amd._lib import MdgenError, launch, lib, ptr
    dev = _cuda()
    buf, out = _guarded(64, torch.int32, SENT_I)
    x = torch.zeros(4, 3, 3, device=dev)
    for cut in (-1.0, float("nan"), float("inf")):
        with pytest.raises(MdgenError, match="cutoff2"):
            launch(lib.mdgen_ens_contact_counts, x, 4, 3, ptr(x), cut, ptr(out))
    with pytest.raises(MdgenError, match="N must be in"):
        launch(lib.mdgen_ens_contact_counts, x, 4, 4097, ptr(x), 64.0, ptr(out))
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    fb, fout = _guarded(64, torch.float64, SENT_F)
    with pytest.raises(MdgenError, match="workspace too small"):
        launch(lib.mdgen_ens_moments, x, 4, 3, ptr(x), ptr(fout), ptr(fout), ptr(ws), 8)
    with pytest.raises(MdgenError, match="Fa and Fb"):
        launch(lib.mdgen_ens_pairwise_d2, x, 0, 4, 3, ptr(x), ptr(x), None, ptr(fout), ptr(ws), 64)
    torch.cuda.synchronize()
    assert (buf == SENT_I).all().item() and (fb == SENT_F).all().item()


# ---- analyze_ensemble ------------------------------------------------------------------------------------------------
def check_analysis(got, traj, ref, aat, **kw):
    """`got` (mdgen_amd.ensemble.analyze_ensemble's dict) key by key against the restatement's, gated by analyze_gates; the contact
    probabilities by the undecided counts, the Jaccard indices by the interval the undecided pairs leave."""
    want, aux = R.analyze_ensemble(traj, ref, aat, with_aux=True, **kw)
    assert set(got) == set(want)
    gates = R.analyze_gates(want, aux)
    for key, gate in gates.items():
        err = np.abs(np.asarray(got[key]) - np.asarray(want[key]))
        print(f"  {key}: worst error {err.max():.3g} (gate {np.max(gate):.3g})")
        assert (err <= gate).all(), key
        assert isinstance(got[key], (float, np.ndarray)), key
    for key, i, n in (("contact_prob", 0, len(traj)), ("ref_contact_prob", 1, len(ref))):
        counts = np.rint(got[key] * n).astype(np.int64)
        assert np.abs(counts / n - got[key]).max() < 1e-12
        assert (np.abs(counts - aux["yes"][i]) <= aux["und"][i]).all(), key
        assert np.array_equal(counts, counts.T) and (np.diag(counts) == n).all()
    for key in ("weak", "transient"):
        lo, hi = aux[key + "_interval"]
        v = got[key + "_contacts_jaccard"]
        assert isinstance(v, float)
        assert (np.isnan(v) and np.isnan(lo)) or lo - 1e-15 <= v <= hi + 1e-15, (key, v, lo, hi)
    return want


@pytest.mark.parametrize("fit", ["heavy", "ca"])
def test_analyze_ensemble(fit):
    from mdgen_amd.ensemble import analyze_ensemble
    traj, ref, aat = R.analyze_case(**R.ANALYZE_CASE)
    got = analyze_ensemble(_dev(traj), ref, aat, fit=fit)
    want = check_analysis(got, traj, ref, aat, fit=fit)
    assert 0.3 < want["rmsf_pearson"] < 1 and want["emd_total"] > 0.1      # the two ensembles differ: the check is not vacuous
    again = analyze_ensemble(traj, _dev(ref), aat, fit=fit)                  # NumPy or device tensors, the same bits
    for key in got:
        assert np.array_equal(got[key], again[key], equal_nan=True), key
    if fit == "ca":
        nopca = analyze_ensemble(_dev(traj), ref, aat, fit=fit, pca=False)
        assert set(got) - set(nopca) == {"pca_w2_ref", "pca_w2_joint", "pca_explained"}
    with pytest.raises(ValueError, match="atom14 slots"):
        analyze_ensemble(_dev(traj), ref, aat[:-1])


def test_pca_fit_against_svd():
    from mdgen_amd.ensemble import pca_fit, pca_project
    traj, ref, aat = R.analyze_case(**R.ANALYZE_CASE)
    ca = np.ascontiguousarray(ref[:, :, R.CA])
    fit, want = pca_fit(_dev(ca), chunk=50), R.pca_fit(ca)
    assert np.allclose(fit["eigenvalues"], want["eigenvalues"], rtol=1e-9, atol=1e-9) and np.allclose(fit["mean"], want["mean"], atol=1e-12)
    assert np.abs(fit["components"][:3] - want["components"][:3]).max() < 1e-8
    assert np.allclose(pca_project(_dev(ca), fit), R.pca_project(ca, want), atol=1e-7)
    with pytest.raises(ValueError, match="3072"):
        pca_fit(torch.zeros(2, 1025, 3, device=_cuda()))


# ---- the command lines, as child processes ---------------------------------------------------------------------------
def _inputs(tmp_path):
    from mdgen_amd.geometry import restype_order
    letters = {v: k for k, v in restype_order.items()}
    data = tmp_path / "data"
    data.mkdir()
    cases = {}
    for i, name in enumerate(("pA", "pB")):
        traj, ref, aat = R.analyze_case(L=8, T=16, F=16, seed=i)
        np.save(data / f"{name}.npy", ref)
        cases[name] = (traj, ref, aat, "".join(letters[int(a)] for a in aat))
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\n" + "".join(f"{n},{c[3]}\n" for n, c in cases.items()))
    return data, split, cases


def _child(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, cwd=str(cwd), env=env, timeout=300)


def test_cli_analyze_ensembles(tmp_path):
    """analyze_ensembles on a two-protein split at 8 residues x 16 frames, one protein from .npy and one from this project's PDB; the
    pickle loads in a process that cannot import this package."""
    from mdgen_amd.pdb import atom14_to_pdb, pdb_to_atom14
    data, split, cases = _inputs(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    np.save(out / "pA.npy", cases["pA"][0])
    atom14_to_pdb(cases["pB"][0], cases["pB"][2], str(out / "pB.pdb"))
    r = _child(["mdgen_amd.analyze_ensembles", "--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--save"], tmp_path)
    assert r.returncode == 0 and "2 of 2 proteins analysed" in r.stdout, r.stderr
    code = ("import sys, pickle; sys.modules['mdgen_amd'] = None; d = pickle.load(open(sys.argv[1], 'rb')); "
            "print(sorted(d), sorted(d['pA'])[:2])")
    r = subprocess.run([sys.executable, "-c", code, str(out / "ensemble.pkl")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.startswith("['pA', 'pB'] ['atom_rmsf', 'ca_rmsf']"), r.stderr
    saved = pickle.load(open(out / "ensemble.pkl", "rb"))
    check_analysis(saved["pA"], cases["pA"][0], cases["pA"][1], cases["pA"][2])
    check_analysis(saved["pB"], pdb_to_atom14(str(out / "pB.pdb"), cases["pB"][2]), cases["pB"][1], cases["pB"][2])


def test_cli_sim_inference_ensemble_superpose(tmp_path):
    """sim_inference --synthetic --analyze --ensemble --superpose on the same split: the pickle carries analyze_ensemble's dict of
    the sampled array, and superposing the written frames again changes nothing beyond the coordinate gate."""
    from mdgen_amd.ensemble import fit_weights
    from mdgen_amd.pdb import pdb_to_atom14
    data, split, cases = _inputs(tmp_path)
    out = tmp_path / "out"
    r = _child(["mdgen_amd.sim_inference", "--synthetic", "--data_dir", str(data), "--split", str(split), "--num_frames", "16",
                "--num_rollouts", "1", "--num_steps", "2", "--batch", "2", "--npy", "--analyze", "--ensemble", "--superpose",
                "--out_dir", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr
    got = pickle.load(open(out / "analysis.pkl", "rb"))
    for name, (_, ref, aat, _) in cases.items():
        assert "JSD" in got[name] and {"ca_rmsf", "contact_prob", "pca_w2_ref", "emd_total"} <= set(got[name]["ensemble"])
        written = np.load(out / f"{name}.npy")
        assert written.shape == (16, 8, 14, 3)
        w, ex = fit_weights(aat, "heavy")
        for frames, slack in ((written, 0.0), (pdb_to_atom14(str(out / f"{name}.pdb"), aat), 0.0005 * 3)):   # (%8.3f: half a unit an axis)
            x = np.asarray(frames, np.float32).reshape(16, -1, 3)
            k = R.kabsch(x, x[0], w)
            moved = np.abs(R.superposed(x, k, ex) - x).max(-1)
            gate = R.coordinate_gate(x, k) + slack
            print(f"  {name}: superposing again moves an atom by at most {moved.max():.3g} (gate {gate.max():.3g})")
            assert (moved <= gate).all()
        assert (x[:, ex == 0] == 0).all()
        # the analysis ran on the tensor the sampler left, before the superposition: the written array is that tensor moved rigidly,
        # frame by frame, with every coordinate within the coordinate gate -- an atom within sqrt(3) x the gate
        x = written.reshape(16, -1, 3)
        moved_by = np.sqrt(3.0) * R.coordinate_gate(x, R.kabsch(x, x[0], w)).max()
        check_analysis(got[name]["ensemble"], written, ref, aat, extra_err=moved_by)
