"""Solvent-accessible surface without a device: the two mdgen_ens_sasa_* bindings against the header, every refusal the library
decides before a launch, the NumPy restatement (tests/sasa_ref.py) and the condition its cases must meet, the host pieces of
mdgen_amd/ensemble.py (sphere points, radii, mutual information, Spearman, the exposed-residue sets) and the command lines."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_ref as R  # noqa: E402
import sasa_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "mdgen_ens_sasa_workspace_bytes": ["A", "P", "bytes"],
    "mdgen_ens_sasa_counts": ["F", "A", "P", "x", "radius", "points", "probe", "counts", "workspace", "workspace_bytes", "stream"]}


def test_header_exports_and_bindings_agree():
    import mdgen_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    kind = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name, want in PARAMS.items():
        decl = re.search(r"int32_t " + name + r"\((.*?)\);", hdr, re.S).group(1)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == want, name
        got = list(getattr(L.lib, name).argtypes)
        for p, a in zip(params, got):
            if "size_t*" in p.replace(" *", "*"):
                assert a is ctypes.POINTER(ctypes.c_size_t), (name, p)
            elif "*" in p:
                assert a is ctypes.c_void_p, (name, p)
            else:
                assert a is kind[p.split()[0]], (name, p)
        assert len(got) == len(params)
        assert L.EXPORTS.count(name) == 1 and getattr(L.lib, name).restype is ctypes.c_int32
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    assert len(L.EXPORTS) == len(set(L.EXPORTS))
    assert "#define MDGEN_ABI_VERSION 8" in hdr and L.lib.mdgen_abi_version() == L.ABI_VERSION == 8   # additions only


def test_kernel_constants_are_the_kernels_and_the_cases_straddle_them():
    from mdgen_amd import ensemble as E
    src = open(os.path.join(ROOT, "mdgen_amd", "csrc", "kernels.h")).read()
    ksrc = open(os.path.join(ROOT, "mdgen_amd", "csrc", "k_ensemble.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    assert E.SASA_NEIGHBOURS == S.NEIGHBOURS == const("kEnsSasaMaxNeighbours")
    assert E.MAX_SASA_POINTS == S.MAX_POINTS == const("kEnsSasaMaxPoints") and E.MAX_ATOMS == const("kEnsMaxAtoms")
    assert float(re.search(r"constexpr float kEnsSasaMaxRadius = ([\d.]+)f;", src).group(1)) == E.MAX_SASA_RADIUS
    # the wave scans 64 atoms and owns 64 points at a time: no other tile in the kernel
    assert E.SASA_SCAN == S.SCAN == 64 and "j0 += 64" in ksrc and "k0 += 64" in ksrc and "lists[kSasaWaves][kEnsSasaMaxNeighbours]" in ksrc
    atoms = {c[1] for c in S.CASES}
    assert {S.SCAN - 1, S.SCAN, S.SCAN + 1} <= atoms and {1, 2, 3584} <= atoms
    points = {c[2] for c in S.CASES + S.POINT_CASES}
    assert {S.SCAN - 1, S.SCAN, S.SCAN + 1, S.MAX_POINTS, 1} <= points
    # an atom of a dense case has A - 1 neighbours: one below the list's capacity, the capacity, one and two above
    assert [a - 1 for a, _ in S.DENSE_CASES] == [S.NEIGHBOURS - 2, S.NEIGHBOURS - 1, S.NEIGHBOURS, S.NEIGHBOURS + 1]
    assert {S.NEIGHBOURS - 1, S.NEIGHBOURS, S.NEIGHBOURS + 1} <= {a for a, _ in S.DENSE_CASES}
    assert S.DENSE_SIDE * np.sqrt(3.0) < 2 * (min(S.BONDI) + S.DENSE_PROBE)
    for a, p in S.DENSE_CASES:
        x, rad, _, _ = S.dense_case(a, p)
        assert (rad > 0).all()
        d = np.linalg.norm(x[0][:, None].astype(np.float64) - x[0][None].astype(np.float64), axis=-1)
        assert d.max() < 2 * (min(S.BONDI) + S.DENSE_PROBE)
    assert S.CASES == [(1, 1, 1, 1.4, 0.0), (2, 2, 7, 1.4, 0.0), (3, 63, 63, 1.4, 0.0), (2, 64, 64, 2.8, 0.0), (2, 65, 65, 1.4, 0.0),
                       (2, 257, 96, 2.8, 0.0), (1, 3584, 15, 2.8, 0.0), (1, 1025, 33, 1.4, 100.0), (5, 56, 960, 1.4, 0.0)]


def test_refusals_without_a_device():
    """Every refusal is decided on the host: a small host buffer stands for every device pointer and is never read; radius and
    points are host arrays and are read.  No call here may pass its checks: it would launch on that buffer."""
    import mdgen_amd._lib as L
    lib, err = L.lib, L.lib.mdgen_last_error
    buf = (ctypes.c_uint8 * 96)()
    p = (ctypes.addressof(buf) + 15) & ~15
    A, P = 5, 7
    rad = np.array([1.7, 0.0, 1.55, 1.52, 1.8], np.float32)
    pts = S.sphere_points(P)
    n = ctypes.c_size_t(12345)

    def call(F=3, A=A, P=P, x=p, radius=None, points=None, probe=1.4, counts=p, ws=p, nbytes=1 << 20):
        radius = rad if radius is None else radius
        points = pts if points is None else points
        rp = None if radius is False else np.ascontiguousarray(radius, np.float32).ctypes.data
        pp = None if points is False else np.ascontiguousarray(points, np.float32).ctypes.data
        return lib.mdgen_ens_sasa_counts(F, A, P, x, rp, pp, probe, counts, ws, nbytes, None)
    for a, q in ((0, 7), (16385, 7), (-1, 7), (5, 0), (5, 4097), (5, -1)):
        assert lib.mdgen_ens_sasa_workspace_bytes(a, q, ctypes.byref(n)) == -2 and n.value == 12345, (a, q)
        assert call(A=a, P=q) == -2, (a, q)
    assert call(A=0) == -2 and b"A must be in 1" in err()
    assert call(A=16385) == -2 and b"A must be in 1" in err()
    assert call(P=0) == -2 and b"P must be in 1" in err()
    assert call(P=4097) == -2 and b"P must be in 1" in err()
    for F in (0, -1, 2 ** 31):
        assert call(F=F) == -2 and b"F must be in 1" in err()
    for bad in (float("nan"), -0.5, 16.5, float("inf")):
        assert call(probe=bad) == -2 and b"probe" in err(), bad
    assert lib.mdgen_ens_sasa_workspace_bytes(5, 7, None) == -1
    for kw in (dict(x=None), dict(radius=False), dict(points=False), dict(counts=None), dict(ws=None)):
        assert call(**kw) == -1 and b"null" in err(), kw
    assert lib.mdgen_ens_sasa_workspace_bytes(A, P, ctypes.byref(n)) == 0 and n.value >= (2 * A + 3 * P) * 4 and n.value % 16 == 0
    need = n.value
    assert call(nbytes=need - 1) == -3 and b"workspace too small" in err()
    assert call(ws=p + 4, nbytes=need) == -2 and b"aligned" in err()
    assert lib.mdgen_ens_sasa_workspace_bytes(16384, 4096, ctypes.byref(n)) == 0 and n.value == (2 * 16384 + 3 * 4096) * 4
    for bad in (-1.0, float("nan"), 16.5, float("inf")):
        r = rad.copy()
        r[3] = bad
        assert call(radius=r, nbytes=need) == -2 and b"radius[3]" in err(), bad
    for k, bad in ((0, (0.0, 0.0, 0.0)), (6, (1.0, 0.1, 0.0)), (2, (float("nan"), 0.0, 1.0)), (3, (float("inf"), 0.0, 0.0)),
                   (4, (0.0, 0.998, 0.0)), (5, (0.0, 0.0, -1.002))):
        q = pts.copy()
        q[k] = bad
        assert call(points=q, nbytes=need) == -2 and f"points[{k}]".encode() in err(), bad


def test_wrappers_refuse_before_a_device_is_needed():
    from mdgen_amd import ensemble as E
    for F, A, P, probe in ((0, 5, 7, 1.4), (2 ** 31, 5, 7, 1.4), (3, 0, 7, 1.4), (3, 16385, 7, 1.4), (3, 5, 0, 1.4), (3, 5, 4097, 1.4),
                           (3, 5, 7, -1.0), (3, 5, 7, float("nan")), (3, 5, 7, 17.0)):
        with pytest.raises(ValueError):
            E._check_sasa_shape(F, A, P, probe)
    E._check_sasa_shape(3, 5, 7, 0.0)
    for n in (0, 4097):
        with pytest.raises(ValueError):
            E.sphere_points(n)
    assert E._sasa_chunk(3584) == (64 << 20) // (4 * 3584) and E._sasa_chunk(3584) * 3584 * 4 <= 64 << 20 and E._sasa_chunk(3584, 7) == 7
    assert E._sasa_chunk(16384) >= 1


# ---- the restatement and its cases -----------------------------------------------------------------------------------
SHARES = {(1, 1025, 33, 1.4, 100.0): 3.7e-5, (5, 56, 960, 1.4, 0.0): 4.6e-6}


@pytest.mark.parametrize("case", S.CASES + S.POINT_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_cases_decide_almost_everything(case):
    x, rad, pts, probe = S.case(*case)
    assert x.dtype == rad.dtype == pts.dtype == np.float32 and (x[:, rad == 0] == 0).all()
    sure, und = S.reference(x, rad, pts, probe)
    share = S.undecided_share(und, rad, len(pts))
    live = rad != 0
    exposed = sure[:, live].sum() / (len(x) * live.sum() * len(pts))
    print(f"undecided share {share:.2e}; exposed share {exposed:.3f}; fully buried atoms {(sure + und == 0)[:, live].sum()}")
    assert share <= S.UNDECIDED_CAP
    if case in S.CASES:
        want = SHARES.get(case, 0.0)
        assert abs(share - want) <= 0.05 * want
    assert (sure[:, ~live] == 0).all() and (und[:, ~live] == 0).all() and (sure + und <= len(pts)).all()
    if case[1] == 1:
        assert (sure == len(pts)).all()
    if case[1] >= 20:
        assert 0.015 <= exposed <= 0.65 and (sure + und == 0)[:, live].any()
    if case[1] <= 257:                                             # the culled reference is the uncull definition
        full = S.reference(x, rad, pts, probe, cull=False)
        assert np.array_equal(full[0], sure) and np.array_equal(full[1], und)
        plain = S.brute_counts(x, rad, pts, probe)
        assert ((sure <= plain) & (plain <= sure + und)).all()


def test_special_cases_stay_under_the_cap():
    for name, (x, rad, pts, probe) in (("clump", S.clump_case()), ("big clump", S.big_clump_case())) + tuple(
            (f"dense {a}", S.dense_case(a, p)) for a, p in S.DENSE_CASES):
        sure, und = S.reference(x, rad, pts, probe)
        share = S.undecided_share(und, rad, len(pts))
        print(f"{name}: undecided share {share:.2e}, exposed points {sure.sum()}")
        assert share <= S.UNDECIDED_CAP and sure.sum() > 0
    x, rad, _, _ = S.clump_case()
    inside = np.linalg.norm(x[0].astype(np.float64) - 20.0, axis=1) <= 1.0 + 1e-5
    assert 290 <= (inside & (rad != 0)).sum() <= 340 and (rad != 0).sum() - (inside & (rad != 0)).sum() == 20
    x, rad, _, _ = S.big_clump_case()
    assert (np.linalg.norm(x[0, :700].astype(np.float64) - 20.0, axis=1) <= 1.5 + 1e-5).all() and (rad != 0).all()
    assert 700 - 1 > S.NEIGHBOURS                                    # every clump atom overflows the list


# ---- the host pieces -------------------------------------------------------------------------------------------------
def test_sphere_points():
    from mdgen_amd.ensemble import sphere_points
    for n in (1, 2, 7, 96, 960, 4096):
        p = sphere_points(n)
        assert p.dtype == np.float32 and p.shape == (n, 3)
        assert np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - 1).max() <= 1e-6
        assert np.array_equal(p, S.sphere_points(n))
        if n >= 96:
            assert np.abs(p.astype(np.float64).mean(0)).max() < 2.0 / n
            d = np.linalg.norm(p[:, None].astype(np.float64) - p[None].astype(np.float64), axis=-1) + 4 * np.eye(n) if n <= 960 else None
            assert d is None or d.min() > 1.5 / np.sqrt(n)          # no two points close together: an even cover
    i = 5
    y = (2 * i + 1) / 96 - 1
    phi = i * (np.pi * (3 - 5 ** 0.5))
    want = (np.cos(phi) * (1 - y * y) ** 0.5, y, np.sin(phi) * (1 - y * y) ** 0.5)
    assert np.array_equal(sphere_points(96)[5], np.array(want).astype(np.float32))


def test_atom_radii():
    from mdgen_amd.ensemble import atom_radii
    from mdgen_amd.geometry import restype_order
    C, N, O, Sx = 1.7, 1.55, 1.52, 1.8
    table = {"G": [N, C, C, O] + [0] * 10,                          # N CA C O
             "C": [N, C, C, O, C, Sx] + [0] * 8,                    # ... CB SG
             "M": [N, C, C, O, C, C, Sx, C] + [0] * 6,              # ... CB CG SD CE
             "D": [N, C, C, O, C, C, O, O] + [0] * 6,               # ... CB CG OD1 OD2
             "K": [N, C, C, O, C, C, C, C, N] + [0] * 5}            # ... CB CG CD CE NZ
    seq = "GCMDK"
    got = atom_radii(np.array([restype_order[c] for c in seq]))
    assert got.dtype == np.float32 and got.shape == (14 * 5,)
    assert np.array_equal(got.reshape(5, 14), np.array([table[c] for c in seq], np.float32))
    every = np.arange(20)
    from mdgen_amd.pdb import residue_tables
    assert np.array_equal(atom_radii(every) != 0, (residue_tables()["atom14_mask"][every] != 0).reshape(-1))
    assert np.array_equal(atom_radii(every), S.atom_radii(every))


def test_sasa_areas_and_residue_matrix():
    from mdgen_amd.ensemble import atom_radii, sasa_areas
    aat = np.array([7, 4, 12, 3, 11])                               # G C M D K
    rad = atom_radii(aat)
    area = sasa_areas(rad, 2.8, 96)
    Rv = (rad + np.float32(2.8)).astype(np.float64)
    assert np.array_equal(area[rad != 0], (4 * np.pi * Rv * Rv / 96)[rad != 0]) and (area[rad == 0] == 0).all()
    side = sasa_areas(rad, 2.8, 96, np.tile(np.arange(14) >= 4, 5))
    m = S.residue_matrix(aat, 2.8, 96, "sidechain")
    assert np.array_equal(m.sum(1), side) and (m[:14] == 0).all()   # glycine: no side chain
    assert np.array_equal(S.residue_matrix(aat, 2.8, 96, "all").sum(1), area)


def test_exposure_mi():
    from mdgen_amd.ensemble import exposure_mi, mi_from_counts
    g = np.random.default_rng(3)
    bits = g.random((200, 7)) < np.array([0.1, 0.5, 0.9, 0.5, 0.3, 0.5, 0.5])
    bits[:, 3] = True                                              # a constant column
    bits[:, 5] = bits[:, 1]                                        # two identical columns
    bits[:, 6] = ~bits[:, 1]                                       # and a complementary one
    got = exposure_mi(bits, chunk=64)
    want = S.mi_loop(bits)
    assert got.shape == (7, 7) and np.abs(got - want).max() <= 1e-12 and np.array_equal(got, got.T)
    assert (got[3] == 0).all() and (got[:, 3] == 0).all()           # a constant shares nothing, and has no entropy
    p = bits[:, 1].mean()
    entropy = -(p * np.log(p) + (1 - p) * np.log(1 - p))
    for v in (got[1, 1], got[1, 5], got[5, 5], got[1, 6]):
        assert abs(v - entropy) <= 1e-12
    assert (got >= -1e-15).all() and got[0, 2] < 0.05
    e = bits.astype(np.float64)
    assert np.array_equal(mi_from_counts(e.T @ e, 200), got)
    import torch
    assert np.array_equal(exposure_mi(torch.from_numpy(bits), chunk=33), got)


def test_spearman():
    from scipy.stats import spearmanr
    from mdgen_amd.ensemble import spearman
    g = np.random.default_rng(4)
    a, b = g.normal(size=50), g.normal(size=50)
    assert abs(spearman(a, b) - spearmanr(a, b)[0]) <= 1e-12
    a, b = g.integers(0, 5, size=60).astype(float), g.integers(0, 4, size=60).astype(float)     # ties
    assert abs(spearman(a, b) - spearmanr(a, b)[0]) <= 1e-12
    assert spearman([1, 2, 3, 4], [10, 20, 25, 400]) == 1.0 and spearman([1, 2, 3, 4], [4, 3, 2, 1]) == -1.0
    assert np.isnan(spearman([1, 1, 1], [1, 2, 3])) and np.isnan(spearman([1, 2, 3], [5, 5, 5]))


def test_exposed_sets_and_jaccard():
    from mdgen_amd.ensemble import TRANSIENT_ABOVE, exposed_sets, jaccard
    assert TRANSIENT_ABOVE == 0.1
    in_ref = np.array([1, 0, 0, 0, 1, 0], bool)
    md = np.array([1.0, 0.5, 0.1, 0.11, 0.05, 0.0])
    sampled = np.array([0.9, 0.05, 0.2, 0.3, 0.5, 0.11])
    a, b = exposed_sets(md, in_ref), exposed_sets(sampled, in_ref)
    assert np.flatnonzero(a).tolist() == [1, 3] and np.flatnonzero(b).tolist() == [2, 3, 5]         # 0.1 itself is outside
    assert jaccard(a, b) == 1 / 4 == R.jaccard_loop(a, b)
    assert np.isnan(jaccard(exposed_sets(md, np.ones(6, bool)), exposed_sets(sampled, np.ones(6, bool))))


def test_analyze_case_decides_every_exposure_bit():
    traj, ref, aat = R.analyze_case(**S.ANALYZE)
    out, aux = S.analyze_sasa(traj, ref, aat, **S.ANALYZE_SETTINGS)
    print(f"undecided points {aux['undecided']}; exposure prob {out['exposure_prob'].min():.2f} .. {out['exposure_prob'].max():.2f}, "
          f"MD {out['ref_exposure_prob'].min():.2f} .. {out['ref_exposure_prob'].max():.2f}; J {out['exposed_residue_jaccard']}; "
          f"rho {out['exposed_mi_spearman']:.3f}")
    assert aux["decided"], "an exposure bit is undecided: change the seed, not the gate"
    atoms = int((S.atom_radii(aat) != 0).sum())
    assert sum(aux["undecided"]) <= S.UNDECIDED_CAP * (33 + 65) * atoms * S.ANALYZE_SETTINGS["n_points"]
    for key in ("exposure_prob", "ref_exposure_prob"):
        live = out[key][np.asarray(aat) != 7]                     # (glycine has no side chain: never exposed)
        assert live.min() < 0.5 and live.max() > 0.9
    assert np.isfinite(out["exposed_mi_spearman"]) and out["exposed_mi"].max() > 0.01


# ---- the command lines -----------------------------------------------------------------------------------------------
def test_analyze_ensembles_cli_passes_the_sasa_options(tmp_path, monkeypatch, capsys):
    from mdgen_amd import analyze_ensembles as cli
    from mdgen_amd import ensemble as E
    p = cli.build_parser()
    base = ["--pdbdir", "o", "--data_dir", "d", "--split", "s.csv"]
    d = p.parse_args(base)
    assert (d.sasa, d.probe, d.sasa_points, d.sasa_threshold, d.sasa_atoms) == (False, 2.8, 960, 2.0, "sidechain")
    assert cli.sasa_options(d) == {}
    a = p.parse_args(base + ["--sasa", "--probe", "1.4", "--sasa_points", "96", "--sasa_threshold", "40", "--sasa_atoms", "all"])
    assert cli.sasa_options(a) == dict(sasa=True, probe=1.4, n_points=96, sasa_threshold=40.0, sasa_atoms="all")
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--sasa_atoms", "backbone"])
    import inspect
    sig = inspect.signature(E.analyze_ensemble).parameters
    assert [sig[k].default for k in ("sasa", "probe", "n_points", "sasa_threshold", "sasa_atoms")] == [False, 2.8, 960, 2.0, "sidechain"]
    assert list(sig)[:6] == ["traj_atom14", "ref_atom14", "aatype", "fit", "cutoff", "pca"]
    seen = []

    def fake(traj, ref, aat, **kw):
        seen.append(kw)
        out = R.analyze_ensemble(traj, ref, aat, kw["fit"], kw["cutoff"], kw["pca"])
        if kw.get("sasa"):
            out.update(S.analyze_sasa(traj, ref, aat, kw["probe"], kw["n_points"], kw["sasa_threshold"], kw["sasa_atoms"], kw["fit"])[0])
        return out
    monkeypatch.setattr(E, "analyze_ensemble", fake)
    traj, ref, aat = R.analyze_case(L=8, T=6, F=8)
    from mdgen_amd.geometry import restype_order
    letters = {v: k for k, v in restype_order.items()}
    out, data = tmp_path / "out", tmp_path / "data"
    out.mkdir()
    data.mkdir()
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\npA," + "".join(letters[int(i)] for i in aat) + "\n")
    np.save(out / "pA.npy", traj)
    np.save(data / "pA.npy", ref)
    common = ["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--no_pca"]
    plain = cli.main(common)
    assert seen[-1] == dict(fit="heavy", cutoff=8.0, pca=False) and "exposed_mi" not in plain["pA"]
    assert "exposed" not in capsys.readouterr().out
    res = cli.main(common + ["--sasa", "--sasa_points", "24", "--sasa_threshold", "40", "--save"])
    assert seen[-1] == dict(fit="heavy", cutoff=8.0, pca=False, sasa=True, probe=2.8, n_points=24, sasa_threshold=40.0, sasa_atoms="sidechain")
    assert "exposed residues J" in capsys.readouterr().out
    new = {"residue_sasa_mean", "ref_residue_sasa_mean", "exposure_prob", "ref_exposure_prob", "exposed_residue_jaccard",
           "exposed_mi", "ref_exposed_mi", "exposed_mi_spearman"}
    assert set(res["pA"]) == set(plain["pA"]) | new
    saved = pickle.load(open(out / "ensemble.pkl", "rb"))
    assert set(saved["pA"]) == set(res["pA"]) and saved["pA"]["exposed_mi"].shape == (8, 8)
    n = len(seen)
    for bad in (["--probe", "-1"], ["--probe", "nan"], ["--sasa_points", "0"], ["--sasa_points", "4097"], ["--sasa_threshold", "inf"]):
        with pytest.raises(SystemExit, match=bad[0].lstrip("-")):
            cli.main(common + ["--sasa"] + bad)
    assert len(seen) == n
    cli.main(common + ["--probe", "-1"])                           # without --sasa its options are not looked at
    assert seen[-1] == dict(fit="heavy", cutoff=8.0, pca=False)


def test_sim_inference_takes_the_sasa_flags_and_defaults_to_off():
    from mdgen_amd import sim_inference
    from mdgen_amd.analyze_ensembles import sasa_options
    s = sim_inference.build_parser().parse_args(["--data_dir", "d"])
    assert not s.sasa and sasa_options(s) == {}
    s = sim_inference.build_parser().parse_args(["--data_dir", "d", "--analyze", "--ensemble", "--sasa", "--probe", "1.4",
                                                 "--sasa_points", "240", "--sasa_threshold", "5", "--sasa_atoms", "all"])
    assert s.ensemble and sasa_options(s) == dict(sasa=True, probe=1.4, n_points=240, sasa_threshold=5.0, sasa_atoms="all")
    src = open(os.path.join(ROOT, "mdgen_amd", "sim_inference.py")).read()
    assert "analyze_ensemble(all_atom14[i], arrs[n], aat, **sasa_options(args))" in src


def test_host_half_imports_without_torch():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; import numpy as np; import mdgen_amd.ensemble as E; "
            "print(E.sphere_points(4).shape, E.atom_radii(np.array([7])).sum() > 6, E.spearman([1, 2, 3], [1, 3, 2]), "
            "E.exposure_mi(np.array([[1, 0], [0, 1]], bool))[0, 1] > 0.69)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "(4, 3) True 0.5 True", r.stderr
