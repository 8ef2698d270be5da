"""mdgen_ens_sasa_counts (csrc/k_ensemble.hip k_sasa) and the chain above it on the GPU against tests/sasa_ref.py (gates: its
docstring).

The counts buffer is pre-filled with a sentinel and has a guard region of the sentinel behind it; the guard must be intact, no
sentinel may be left where a count belongs, and a second call gives the same integers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_ref as R  # noqa: E402
import sasa_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
SENT_I = -77777


def _cuda():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(_cuda())


def run_counts(x, rad, pts, probe):
    """The device's counts int64 [F, A] of one call, checked for the guard, the sentinel and a second call's integers."""
    from mdgen_amd.ensemble import sasa_counts_into, sasa_workspace_bytes
    F, A = x.shape[:2]
    xd = _dev(x)
    ws = torch.empty(sasa_workspace_bytes(A, len(pts)), dtype=torch.uint8, device=_cuda())
    got = []
    for _ in range(2):
        buf = torch.full((F * A + GUARD,), SENT_I, dtype=torch.int32, device=_cuda())
        sasa_counts_into(xd, rad, pts, probe, buf[:F * A], ws)
        torch.cuda.synchronize()
        assert (buf[F * A:] == SENT_I).all().item(), "guard overwritten"
        assert not (buf[:F * A] == SENT_I).any().item(), "a count was not written"
        got.append(buf[:F * A].cpu().numpy().reshape(F, A).astype(np.int64))
    assert np.array_equal(got[0], got[1]), "a second call gave other integers"
    return got[0]


def check_counts(x, rad, pts, probe):
    sure, und = S.reference(x, rad, pts, probe)
    assert S.undecided_share(und, rad, len(pts)) <= S.UNDECIDED_CAP
    got = run_counts(x, rad, pts, probe)
    print(f"  undecided points {und.sum()}; entries off the sure count {(got != sure).sum()} of {got.size}")
    assert ((sure <= got) & (got <= sure + und)).all(), np.argwhere((got < sure) | (got > sure + und))[:5]
    assert (got[und == 0] == sure[und == 0]).all()
    assert (got[:, np.asarray(rad) == 0] == 0).all()
    return got


@pytest.mark.parametrize("case", S.CASES + S.POINT_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_counts(case):
    check_counts(*S.case(*case))


@pytest.mark.parametrize("A,P", S.DENSE_CASES)
def test_neighbour_list_at_its_capacity(A, P):
    """Every atom has A - 1 neighbours: 510 and 511 fit the list of 512, 512 fills it, 513 overflows it into the scan of all atoms."""
    check_counts(*S.dense_case(A, P))


def test_clumps_fall_back_to_the_scan_of_all_atoms():
    check_counts(*S.clump_case())                                  # ~300 atoms within 1 A, 20 scattered
    got = check_counts(*S.big_clump_case())                         # 700 within 1.5 A: more than the list holds
    assert got[0, 700:].max() > 0


def test_lone_far_and_absent_atoms():
    pts = S.sphere_points(97)
    one = np.array([[[3.0, -2.0, 5.0]]], np.float32)
    assert run_counts(one, np.array([1.7], np.float32), pts, 1.4).tolist() == [[97]]
    g = np.random.default_rng(1)
    far = (np.arange(70)[None, :, None] * np.array([40.0, 0.0, 0.0]) + g.random((2, 70, 3))).astype(np.float32)
    rad = g.choice(np.array(S.BONDI), 70).astype(np.float32)
    assert (run_counts(far, rad, pts, 2.8) == 97).all()            # 40 A apart: nothing reaches anything
    x, _, _, _ = S.case(2, 65, 65, 1.4, 0.0)
    assert (run_counts(x, np.zeros(65, np.float32), pts, 1.4) == 0).all()      # no atom at all: nothing is read as one
    # a small atom at the centre of a large one: wholly buried, and none of the large one's points lies inside it
    pair = np.array([[[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]], np.float32)
    assert run_counts(pair, np.array([4.0, 1.0], np.float32), pts, 1.4).tolist() == [[97, 0]]
    assert run_counts(pair, np.array([4.0, 1.0], np.float32), pts, 0.0).tolist() == [[97, 0]]


def test_padding_slots_are_no_atoms_at_the_origin():
    from mdgen_amd.ensemble import atom_radii
    traj, _, aat = R.analyze_case(L=6, T=3, F=2, seed=1)
    x = traj.reshape(3, -1, 3).copy()
    rad = atom_radii(aat)
    assert (rad == 0).any() and (x[:, rad == 0] == 0).all()
    x[:, rad != 0] -= x[:, rad != 0].mean(1, keepdims=True)        # the molecule sits on the origin, where the padding slots are
    pts = S.sphere_points(96)
    got = check_counts(x, rad, pts, 1.4)
    live = rad != 0
    assert (got[:, ~live] == 0).all()
    alone = run_counts(np.ascontiguousarray(x[:, live]), rad[live], pts, 1.4)            # the same atoms without the padding slots
    assert np.array_equal(got[:, live], alone)
    ghosts = run_counts(x, np.where(live, rad, np.float32(1.7)), pts, 1.4)               # real atoms at the origin do bury
    assert ghosts[:, live].sum() < got[:, live].sum()


def test_a_frames_counts_do_not_depend_on_where_it_stands():
    from mdgen_amd.ensemble import sasa_counts
    x, rad, pts, probe = S.case(65, 56, 64, 1.4, 0.0)
    many = run_counts(x, rad, pts, probe)
    first = run_counts(np.ascontiguousarray(x[64:]), rad, pts, probe)                  # frame 64: last of 65, and first of 1
    assert np.array_equal(first[0], many[64])
    xd = _dev(x)
    whole = sasa_counts(xd, rad, n_points=64, probe=probe)
    assert whole.dtype == torch.int32 and whole.shape == (65, 56) and whole.is_cuda
    assert np.array_equal(whole.cpu().numpy(), many)
    for chunk in (1, 7, 64):                                       # frame 64 falls in chunks of other sizes and places
        assert torch.equal(sasa_counts(xd, rad, n_points=64, probe=probe, chunk=chunk), whole)
    assert torch.equal(sasa_counts(xd.reshape(65, 4, 14, 3), rad, n_points=64, probe=probe), whole)


def test_wrapper_refusals_leave_the_counts_untouched():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.ensemble import sasa_counts_into, sasa_workspace_bytes
    x, rad, pts, probe = S.case(2, 20, 63, 1.4, 0.0)
    xd = _dev(x)
    buf = torch.full((2 * 20 + GUARD,), SENT_I, dtype=torch.int32, device=_cuda())
    ws = torch.empty(sasa_workspace_bytes(20, 63), dtype=torch.uint8, device=_cuda())
    bad_r, bad_p = rad.copy(), pts.copy()
    bad_r[3], bad_p[5] = np.nan, (0.5, 0.5, 0.5)
    for r, p, w in ((bad_r, pts, ws), (rad, bad_p, ws), (rad, pts, ws[:-16])):
        with pytest.raises(MdgenError, match="radius|unit vector|workspace too small"):
            sasa_counts_into(xd, r, p, probe, buf[:40], w)
    with pytest.raises(ValueError):
        sasa_counts_into(xd, rad[:19], pts, probe, buf[:40], ws)
    with pytest.raises(ValueError):
        sasa_counts_into(xd, rad, pts, probe, buf[:39], ws)
    torch.cuda.synchronize()
    assert (buf == SENT_I).all().item()


def test_residue_sasa_is_the_counts_times_the_areas():
    from mdgen_amd.ensemble import atom_radii, residue_sasa, sasa_counts
    traj, _, aat = R.analyze_case(L=6, T=5, F=2, seed=1)
    xd = _dev(traj)
    rad = atom_radii(aat)
    counts = sasa_counts(xd, rad, n_points=96, probe=2.8).cpu().numpy().astype(np.float64)
    for atoms in ("sidechain", "all"):
        got = residue_sasa(xd, aat, atoms=atoms, probe=2.8, n_points=96)
        assert got.dtype == torch.float64 and got.shape == (5, 6) and got.is_cuda
        want = counts @ S.residue_matrix(aat, 2.8, 96, atoms)
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-12 * want.max()
        if atoms == "sidechain":
            assert (got.cpu().numpy()[:, np.asarray(aat) == 7] == 0).all()       # glycine
    with pytest.raises(ValueError, match="sidechain"):
        residue_sasa(xd, aat, atoms="backbone")


# ---- analyze_ensemble ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _analyze():
    from mdgen_amd.ensemble import analyze_ensemble
    traj, ref, aat = R.analyze_case(**S.ANALYZE)
    want, aux = S.analyze_sasa(traj, ref, aat, **S.ANALYZE_SETTINGS)
    plain = analyze_ensemble(_dev(traj), _dev(ref), aat)
    got = analyze_ensemble(_dev(traj), _dev(ref), aat, sasa=True, **S.ANALYZE_SETTINGS)
    return want, aux, plain, got


def test_analyze_ensemble_sasa_against_the_restatement():
    want, aux, plain, got = _analyze()
    assert aux["decided"], "an exposure bit is undecided: change the seed, not the gate"
    new = ["residue_sasa_mean", "ref_residue_sasa_mean", "exposure_prob", "ref_exposure_prob", "exposed_residue_jaccard", "exposed_mi",
           "ref_exposed_mi", "exposed_mi_spearman"]
    assert list(got) == list(plain) + new                         # after the existing keys, in this order
    for key in ("exposure_prob", "ref_exposure_prob"):
        assert np.array_equal(got[key], want[key]), key
    assert got["exposed_residue_jaccard"] == want["exposed_residue_jaccard"] or (
        np.isnan(got["exposed_residue_jaccard"]) and np.isnan(want["exposed_residue_jaccard"]))
    for key in ("exposed_mi", "ref_exposed_mi"):
        assert got[key].shape == (12, 12) and np.abs(got[key] - want[key]).max() <= 1e-12, key
    assert abs(got["exposed_mi_spearman"] - want["exposed_mi_spearman"]) <= 1e-12
    for key, lo, hi in (("residue_sasa_mean", aux["lo"][0], aux["hi"][0]), ("ref_residue_sasa_mean", aux["lo"][1], aux["hi"][1])):
        slack = 1e-9 * hi.mean(0).max()
        print(f"  {key}: {got[key].min():.1f} .. {got[key].max():.1f} A^2, the undecided points' area up to {(hi - lo).mean(0).max():.2e}")
        assert (lo.mean(0) - slack <= got[key]).all() and (got[key] <= hi.mean(0) + slack).all(), key
    for v in got.values():
        assert isinstance(v, (float, np.ndarray))


def test_exposure_bits_sets_and_joint_counts_are_exact():
    from mdgen_amd.ensemble import atom_radii, exposed_sets, residue_sasa, superpose
    want, aux, _, got = _analyze()
    traj, ref, aat = R.analyze_case(**S.ANALYZE)
    w, ex = R.fit_weights(aat, "heavy")
    target = _dev(ref)[0].reshape(-1, 3).clone()
    for n, (coords, prob_key) in enumerate(((traj, "exposure_prob"), (ref, "ref_exposure_prob"))):
        xs = superpose(_dev(coords), target, weights=torch.from_numpy(w.astype(np.float32)), exists=ex)
        area = residue_sasa(xs, aat, atoms="sidechain", probe=2.8, n_points=96).cpu().numpy()
        bits = area > 40.0
        assert np.array_equal(bits, aux["bits"][n])
        assert ((aux["lo"][n] - 1e-9 <= area) & (area <= aux["hi"][n] + 1e-9)).all()
        e = bits.astype(np.int64)
        assert np.array_equal(e.T @ e, aux["n11"][n])
        if n == 1:
            in_ref = bits[0]
            assert np.array_equal(exposed_sets(got["ref_exposure_prob"], in_ref), aux["sets"][0])
            assert np.array_equal(exposed_sets(got["exposure_prob"], in_ref), aux["sets"][1])
    assert (atom_radii(aat) != 0).sum() == ex.sum()


def test_without_sasa_the_key_set_is_todays():
    _, _, plain, _ = _analyze()
    assert list(plain) == ["atom_rmsf", "ref_atom_rmsf", "ca_rmsf", "ref_ca_rmsf", "rmsf_pearson", "mean_pairwise_rmsd", "rms_pairwise_rmsd",
                           "ref_mean_pairwise_rmsd", "ref_rms_pairwise_rmsd", "cross_mean_pairwise_rmsd", "cross_rms_pairwise_rmsd",
                           "emd_mean", "emd_var", "emd_total", "contact_prob", "ref_contact_prob", "weak_contacts_jaccard",
                           "transient_contacts_jaccard", "pca_w2_ref", "pca_w2_joint", "pca_explained"]
    assert set(plain) == set(R.analyze_ensemble(*R.analyze_case(L=8, T=4, F=4)))
