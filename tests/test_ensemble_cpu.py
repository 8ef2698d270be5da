"""Ensemble statistics without a device: the mdgen_ens_* bindings against the header, every refusal the library decides before a
launch, the NumPy restatement (tests/ensemble_ref.py) against independent formulas, the well-posedness of its cases, the host
estimators of mdgen_amd/ensemble.py, and the command line's argument handling and skip-and-name behaviour."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "mdgen_ens_superpose": ["F", "A", "x", "ref", "w", "exists", "out", "rot", "rmsd", "stream"],
    "mdgen_ens_moments_workspace_bytes": ["F", "A", "bytes"],
    "mdgen_ens_moments": ["F", "A", "x", "mean", "cov", "workspace", "workspace_bytes", "stream"],
    "mdgen_ens_pairwise_d2_workspace_bytes": ["Fa", "Fb", "A", "bytes"],
    "mdgen_ens_pairwise_d2": ["Fa", "Fb", "A", "xa", "xb", "d2", "sums", "workspace", "workspace_bytes", "stream"],
    "mdgen_ens_contact_counts": ["F", "N", "ca", "cutoff2", "counts", "stream"]}


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
    assert len(L.EXPORTS) == len(set(L.EXPORTS))
    assert "#define MDGEN_ABI_VERSION 8" in hdr and L.lib.mdgen_abi_version() == L.ABI_VERSION == 8   # additions only
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in PARAMS:
        assert name in doc, name
    from mdgen_amd import build
    assert "k_ensemble.hip" in build.SOURCES and "ensemble.h" in build.HEADERS


def test_tile_constants_are_the_kernels_and_the_cases_straddle_them():
    from mdgen_amd import ensemble as E
    src = open(os.path.join(ROOT, "mdgen_amd", "csrc", "kernels.h")).read()
    ksrc = open(os.path.join(ROOT, "mdgen_amd", "csrc", "k_ensemble.hip")).read()

    def const(name, text=src):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert (E.PAIR_TILE_A, E.PAIR_TILE_B, E.PAIR_CHUNK) == (const("kEnsPairTileA"), const("kEnsPairTileB"), const("kEnsPairChunk"))
    assert (E.WAVE_ATOMS, E.MAX_ATOMS, E.MAX_RESIDUES) == (const("kEnsWaveAtoms"), const("kEnsMaxAtoms"), const("kEnsMaxResidues"))
    assert E.CONTACT_TILE == const("kCcTile", ksrc)
    fa = {c[0] for c in R.PAIRWISE_CASES}
    fb = {c[1] if c[1] is not None else c[0] for c in R.PAIRWISE_CASES}
    coords = {3 * c[2] for c in R.PAIRWISE_CASES}
    for edge, have in ((E.PAIR_TILE_A, fa), (E.PAIR_TILE_B, fb)):
        assert {edge - 1, edge, edge + 1} <= have, (edge, sorted(have))
    assert {E.PAIR_CHUNK - 3, E.PAIR_CHUNK, E.PAIR_CHUNK + 3} <= coords          # (3 A: the nearest below and above)
    atoms = {c[1] for c in R.SUPERPOSE_CASES}
    assert {63, 64, 65} <= atoms and min(atoms) == 3 and any(a <= E.WAVE_ATOMS for a in atoms) and any(a > E.WAVE_ATOMS for a in atoms)
    n = {c[1] for c in R.CONTACT_CASES}
    assert {E.CONTACT_TILE - 1, E.CONTACT_TILE, E.CONTACT_TILE + 1} <= n
    for must in ((1, 3), (2, 4), (65, 56), (3, 63), (3, 64), (3, 65), (257, 257), (5, 3584), (4099, 56)):
        assert must in {c[:2] for c in R.SUPERPOSE_CASES}
    assert {c[:2] for c in R.MOMENTS_CASES} == {(1, 1), (2, 3), (65, 56), (257, 65), (4099, 257), (100003, 4)}
    assert any(c[2] == 100.0 for c in R.MOMENTS_CASES)
    for must in ((1, 1, 1), (2, 3, 1), (63, 65, 3), (64, 64, 4), (65, 129, 56), (257, 250, 256), (250, 250, 1024), (65, None, 56),
                 (257, None, 256)):
        assert must in R.PAIRWISE_CASES
    assert R.CONTACT_CASES == [(1, 1), (1, 2), (3, 63), (3, 65), (65, 64), (257, 257), (17, 1024)]


def test_refusals_without_a_device():
    """Every refusal is decided on the host, the shape before the pointers: a small host buffer stands for every device pointer and
    is never read.  No call here may pass its checks: it would launch on that buffer."""
    import mdgen_amd._lib as L
    lib, err = L.lib, L.lib.mdgen_last_error
    buf = (ctypes.c_uint8 * 96)()
    p = (ctypes.addressof(buf) + 15) & ~15                        # 16-byte aligned, so that p + 4 and p + 8 surely are not
    n = ctypes.c_size_t(12345)
    # superpose: shapes, then nulls (w is only read after both)
    for F, A in ((0, 56), (-1, 56), (2 ** 40 + 1, 56), (5, 2), (5, 0), (5, 16385)):
        assert lib.mdgen_ens_superpose(F, A, p, p, p, None, p, None, None, None) == -2, (F, A)
        assert lib.mdgen_ens_superpose(F, A, None, None, None, None, None, None, None, None) == -2
    assert lib.mdgen_ens_superpose(5, 2, p, p, p, None, p, None, None, None) == -2 and b"A must be in 3" in err()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        x, ref, w, out = args
        assert lib.mdgen_ens_superpose(5, 56, x, ref, w, None, out, None, None, None) == -1 and b"null" in err()
    # moments
    for F, A in ((0, 4), (2 ** 40 + 1, 4), (5, 0), (5, 16385)):
        assert lib.mdgen_ens_moments(F, A, p, p, p, p, 1 << 30, None) == -2, (F, A)
        assert lib.mdgen_ens_moments_workspace_bytes(F, A, ctypes.byref(n)) == -2 and n.value == 12345
    assert lib.mdgen_ens_moments_workspace_bytes(5, 4, None) == -1
    assert lib.mdgen_ens_moments_workspace_bytes(100003, 4, ctypes.byref(n)) == 0 and 0 < n.value <= 19 << 20
    need = n.value
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.mdgen_ens_moments(100003, 4, *args, need, None) == -1
    assert lib.mdgen_ens_moments(100003, 4, p, p, p, p, need - 1, None) == -3 and b"workspace too small" in err()
    assert lib.mdgen_ens_moments(100003, 4, p, p, p, p + 4, need, None) == -2 and b"aligned" in err()
    assert lib.mdgen_ens_moments_workspace_bytes(2 ** 40, 16384, ctypes.byref(n)) == 0 and n.value <= 19 << 20
    # pairwise
    for Fa, Fb, A in ((0, 5, 4), (5, 0, 4), (2 ** 20, 5, 4), (5, 2 ** 20, 4), (5, 5, 0), (5, 5, 16385)):
        assert lib.mdgen_ens_pairwise_d2(Fa, Fb, A, p, p, p, p, p, 1 << 30, None) == -2, (Fa, Fb, A)
        n.value = 12345
        assert lib.mdgen_ens_pairwise_d2_workspace_bytes(Fa, Fb, A, ctypes.byref(n)) == -2 and n.value == 12345
    assert lib.mdgen_ens_pairwise_d2_workspace_bytes(2 ** 20 - 1, 2 ** 20 - 1, 16384, ctypes.byref(n)) == 0 and n.value <= 1 << 20
    assert lib.mdgen_ens_pairwise_d2_workspace_bytes(250, 250, 256, ctypes.byref(n)) == 0 and n.value > 0
    need = n.value
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        xa, xb, sums, ws = args
        assert lib.mdgen_ens_pairwise_d2(250, 250, 256, xa, xb, None, sums, ws, need, None) == -1
    assert lib.mdgen_ens_pairwise_d2(250, 250, 256, p, p, None, p, p, need - 1, None) == -3
    assert lib.mdgen_ens_pairwise_d2(250, 250, 256, p, p, None, p, p + 8, need, None) == -2
    # contacts
    for F, N in ((0, 8), (2 ** 31, 8), (5, 0), (5, 4097)):
        assert lib.mdgen_ens_contact_counts(F, N, p, 64.0, p, None) == -2, (F, N)
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        assert lib.mdgen_ens_contact_counts(5, 8, p, bad, p, None) == -2 and b"cutoff2" in err(), bad
    assert lib.mdgen_ens_contact_counts(5, 8, None, 64.0, p, None) == -1
    assert lib.mdgen_ens_contact_counts(5, 8, p, 64.0, None, None) == -1


def test_wrappers_refuse_before_a_device_is_needed():
    from mdgen_amd import ensemble as E
    for F, A, m in ((0, 5, 1), (5, 2, 3), (5, 16385, 1), (2 ** 40 + 1, 5, 1)):
        with pytest.raises(ValueError):
            E._check_frames_atoms(F, A, m)
    for shape in ((0, 5, 4), (5, 2 ** 20, 4), (5, 5, 0)):
        with pytest.raises(ValueError):
            E._check_pairwise_shape(*shape)
    for F, N, c in ((0, 8, 8.0), (5, 4097, 8.0), (5, 8, -1.0), (5, 8, float("nan")), (5, 8, float("inf"))):
        with pytest.raises(ValueError):
            E._check_contact_shape(F, N, c)
    assert E.cutoff2_f32(8.0) == np.float32(64.0) and float(E.cutoff2_f32(0.1)) == float(np.float32(0.1 * 0.1)) == R.cutoff2(0.1)
    with pytest.raises(ValueError, match="heavy"):
        E.fit_weights(np.array([0, 1]), "all")
    w, ex = E.fit_weights(np.array([7, 0, 17]), "heavy")           # GLY 4, ALA 5, TRP 14 atoms
    assert w.dtype == np.float32 and ex.dtype == np.uint8 and w.sum() == 4 + 5 + 14 and np.array_equal(w != 0, ex != 0)
    w, ex2 = E.fit_weights(np.array([7, 0, 17]), "ca")
    assert np.flatnonzero(w).tolist() == [1, 15, 29] and np.array_equal(ex, ex2)
    rw, rex = R.fit_weights(np.array([7, 0, 17]), "heavy")
    assert np.array_equal(rw, E.fit_weights(np.array([7, 0, 17]), "heavy")[0]) and np.array_equal(rex, ex)


# ---- the restatement against independent formulas --------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SUPERPOSE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_superpose_cases_are_well_posed_and_kabsch_minimises(case):
    x, ref, w, exists = R.superpose_case(*case)
    assert x.dtype == ref.dtype == w.dtype == np.float32 and (w >= 0).all() and (w > 0).sum() >= 3
    if case[2] == "three":
        assert (w > 0).sum() == 3
    k = R.kabsch(x, ref, w)
    wp = R.well_posedness(k)
    print(f"well-posedness min {wp.min():.3g}; rotation gate max {R.rotation_gate(k).max():.3g}; frames with det H < 0: {(k['d'] < 0).sum()}")
    assert (wp >= R.WELL_POSED).all() and R.rotation_gate(k).max() <= 2.3e-10
    assert np.abs(np.linalg.det(k["R"]) - 1).max() < 1e-12
    assert np.abs(np.einsum("fij,fkj->fik", k["R"], k["R"]) - np.eye(3)).max() < 1e-12
    F = case[0]
    if F > 5 and case[2] != "three":
        assert k["d"][5] < 0                                      # the mirror frame: a proper rotation all the same
    if F > 1:
        assert k["rmsd"][0] < 1e-12 and np.abs(k["R"][0] - np.eye(3)).max() < 1e-12
    g = np.random.default_rng(7)
    for f in sorted({0, min(5, F - 1), F - 1}):
        best = R.objective(k["R"][f], x[f], ref, w, k["cx"][f], k["cr"])
        assert abs(best - k["rmsd"][f] ** 2 * w.astype(np.float64).sum()) <= 1e-9 * max(best, 1e-9)
        for _ in range(100):
            assert R.objective(R.random_rotation(g), x[f], ref, w, k["cx"][f], k["cr"]) >= best - 1e-9 * max(best, 1.0)
        for _ in range(20):                                       # and against rotations close to the optimum
            q = R.random_rotation(g)
            near = k["R"][f] @ (np.eye(3) + 1e-3 * (q - q.T))
            u, _, vt = np.linalg.svd(near)
            assert R.objective(u @ vt, x[f], ref, w, k["cx"][f], k["cr"]) >= best - 1e-9 * max(best, 1.0)
    if exists is not None:
        assert (exists == 0).any() and (x[:, exists == 0] == 0).all() and (w[exists == 0] == 0).all()


@pytest.mark.parametrize("F,A,offset", R.MOMENTS_CASES)
def test_moments_restatement(F, A, offset):
    x = R.moments_case(F, A, offset)
    mean, cov = R.moments(x)
    x64 = x.astype(np.float64)
    assert np.allclose(mean, x64.sum(0) / F, rtol=1e-12, atol=1e-12)
    if F > 1:
        want = np.stack([np.cov(x64[:, a].T, bias=True) for a in range(min(A, 5))])
        assert np.allclose(cov[:min(A, 5)], want.reshape(-1, 3, 3), rtol=1e-10, atol=1e-12)
    else:
        assert (cov == 0).all()
    mg, cg = R.moments_gates(x)
    assert mg.shape == (A, 3) and cg.shape == (A, 3, 3) and (mg >= 0).all() and (cg >= 0).all()
    if offset:
        assert np.abs(mean).min() > 50


@pytest.mark.parametrize("F,N", R.CONTACT_CASES)
def test_contact_cases_decide_almost_everything(F, N):
    ca = R.contact_case(F, N)
    yes, und = R.contact_reference(ca)
    share = und.sum() / (F * N * N)
    off = ~np.eye(N, dtype=bool)
    frac = yes[off].sum() / max(1, F * off.sum())
    print(f"undecided share {share:.2e}; pairs in contact {frac:.3f}")
    assert share <= R.UNDECIDED_CAP and np.array_equal(yes, yes.T) and (np.diag(yes) == F).all()
    if N >= 63:
        assert 0.15 < frac < 0.25
    d = np.linalg.norm(ca[0, :, None].astype(np.float64) - ca[0, None].astype(np.float64), axis=-1)     # frame 0 by another formula
    y0, u0 = R.contact_reference(ca[:1])
    assert np.array_equal((d < 8.0) & (u0 == 0), (y0 > 0) & (u0 == 0))


def test_pairwise_restatement():
    xa, xb = R.pairwise_case(5, 7, 4)
    d2 = R.pairwise_d2(xa, xb)
    a, b = xa.reshape(5, -1).astype(np.float64), xb.reshape(7, -1).astype(np.float64)
    gram = (a * a).sum(1)[:, None] + (b * b).sum(1)[None] - 2 * a @ b.T
    assert np.allclose(d2, gram, rtol=1e-10, atol=1e-9)
    s = R.pairwise_sums(d2, 4)
    assert np.isclose(s[0], sum(np.sqrt(v / 4) for v in d2.ravel())) and np.isclose(s[1], d2.sum() / 4)
    assert (np.diag(R.pairwise_d2(xa, xa)) == 0).all()


# ---- the host estimators ---------------------------------------------------------------------------------------------
def test_gaussian_w2():
    from mdgen_amd.ensemble import gaussian_w2
    g = np.random.default_rng(3)
    m = g.normal(size=(6, 3))
    a = g.normal(size=(6, 3, 3))
    cov = a @ np.swapaxes(a, -1, -2)
    t, v, total = gaussian_w2(m, cov, m, cov)                      # equal Gaussians
    assert (t == 0).all() and np.abs(v).max() < 1e-12 and total < 1e-6
    sa, sb = g.random(6) + 0.5, g.random(6) + 0.5                  # isotropic: (sa - sb)^2 * 3
    eye = np.eye(3)[None]
    t, v, total = gaussian_w2(m, sa[:, None, None] ** 2 * eye, m + 1.0, sb[:, None, None] ** 2 * eye)
    assert np.allclose(t, 3.0) and np.allclose(v, 3 * (sa - sb) ** 2, rtol=1e-10, atol=1e-12)
    assert np.isclose(total, np.sqrt(np.mean(3.0 + 3 * (sa - sb) ** 2)))
    b = g.normal(size=(6, 3, 3))
    cov_b = b @ np.swapaxes(b, -1, -2)
    cov_b[0] = np.outer(b[0, 0], b[0, 0])                          # a singular covariance
    got, want = gaussian_w2(m, cov, m + 0.5, cov_b), R.gaussian_w2(m, cov, m + 0.5, cov_b)
    for u, w in zip(got, want):
        assert np.allclose(u, w, rtol=1e-9, atol=1e-10)
    assert (got[1] >= 0).all()


def test_pca_w2_and_jaccard():
    from mdgen_amd.ensemble import contact_sets, jaccard, pca_w2, pearson
    g = np.random.default_rng(5)
    a = g.normal(size=(40, 2))
    assert pca_w2(a, a[g.permutation(40)]) == 0.0
    b = g.normal(size=(101, 2))
    assert pca_w2(a, b) == R.pca_w2(a, b) > 0
    picked = b[np.round(np.linspace(0, 100, 40)).astype(int)]
    assert np.isclose(pca_w2(a, b), pca_w2(a, picked))
    assert np.isclose(pca_w2(a, a + np.array([3.0, 4.0])), 5.0)
    x, y = np.array([1, 1, 0, 0], bool), np.array([1, 0, 1, 0], bool)
    assert jaccard(x, y) == 1 / 3 == R.jaccard_loop(x, y) and jaccard(x, x) == 1.0 and jaccard(x, ~x) == 0.0
    assert np.isnan(jaccard(np.zeros(4, bool), np.zeros(4, bool))) and np.isnan(R.jaccard_loop([0, 0], [0, 0]))
    prob = np.array([[1.0, 0.95, 0.5, 0.05], [0.95, 1.0, 0.89, 0.11], [0.5, 0.89, 1.0, 0.1], [0.05, 0.11, 0.1, 1.0]])
    in_ref = np.array([[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 1]], bool)
    weak, trans = contact_sets(prob, in_ref)
    assert np.argwhere(weak).tolist() == [[0, 2], [1, 2]] and np.argwhere(trans).tolist() == [[1, 3]]   # 0.9 and 0.1 are outside
    assert np.isclose(pearson([1, 2, 3, 5], [2, 4, 6, 11]), np.corrcoef([1, 2, 3, 5], [2, 4, 6, 11])[0, 1])
    assert R.jaccard_interval((x, x), (y, y)) == (1 / 3, 1 / 3)
    lo, hi = R.jaccard_interval((x, x | y), (y, y))
    assert lo <= 1 / 3 <= hi and lo < hi


def test_pca_restatement_against_the_covariance_eigenproblem():
    g = np.random.default_rng(11)
    ca = (g.normal(size=(50, 4, 3)) * np.array([3.0, 2.0, 1.0])).astype(np.float32)
    fit = R.pca_fit(ca)
    y = ca.reshape(50, -1).astype(np.float64)
    c = np.cov(y.T, bias=True)
    lam, v = np.linalg.eigh(c)
    assert np.allclose(fit["eigenvalues"], lam[::-1], rtol=1e-10, atol=1e-12) and np.isclose(fit["explained"].sum(), 1.0)
    for i in range(3):
        comp = fit["components"][i]
        assert abs(abs(comp @ v[:, -1 - i]) - 1) < 1e-9 and comp[np.abs(comp).argmax()] > 0
    proj = R.pca_project(ca, fit)
    assert np.allclose(proj.var(0), lam[::-1][:2], rtol=1e-10)


def test_analyze_restatement_is_self_consistent():
    traj, ref, aat = R.analyze_case(**R.ANALYZE_CASE)
    assert traj.shape == (33, 8, 14, 3) and ref.shape == (129, 8, 14, 3)
    out, aux = R.analyze_ensemble(traj, ref, aat, with_aux=True)
    same = R.analyze_ensemble(ref, ref, aat)
    assert same["emd_total"] < 1e-6 and abs(same["rmsf_pearson"] - 1) < 1e-12
    assert same["weak_contacts_jaccard"] == 1.0 or np.isnan(same["weak_contacts_jaccard"])
    assert abs(same["mean_pairwise_rmsd"] - same["cross_mean_pairwise_rmsd"]) < 1e-12 and same["pca_w2_ref"] < 1e-9
    gates = R.analyze_gates(out, aux)
    assert set(gates) == set(out) - {"contact_prob", "ref_contact_prob", "weak_contacts_jaccard", "transient_contacts_jaccard"}
    assert all(np.all(np.asarray(g) > 0) for g in gates.values()) and aux["g"] < 1e-3
    share = sum(int(u.sum()) for u in aux["und"]) / ((33 + 129 + 1) * 64)
    assert share <= 0.05                                          # (64 pairs a frame: a handful of near-cutoff ones at the most)
    rot = R.random_rotation(np.random.default_rng(2))             # rigid motion of the sampled ensemble changes nothing
    moved = (traj.astype(np.float64) @ rot.T + 5.0).astype(np.float32)
    moved[:, np.asarray(R.fit_weights(aat, "heavy")[1]).reshape(8, 14) == 0] = 0.0
    again = R.analyze_ensemble(moved, ref, aat)
    for key in ("ca_rmsf", "mean_pairwise_rmsd", "emd_total", "pca_w2_ref"):
        assert np.allclose(again[key], out[key], rtol=0, atol=1e-4), key


# ---- the command line ------------------------------------------------------------------------------------------------
def test_analyze_ensembles_cli_skips_and_names(tmp_path, monkeypatch, capsys):
    from mdgen_amd import analyze_ensembles as cli
    from mdgen_amd import ensemble as E
    p = cli.build_parser()
    d = p.parse_args(["--pdbdir", "o", "--data_dir", "d", "--split", "s.csv"])
    assert (d.suffix, d.ref_suffixes, d.fit, d.no_pca, d.save, d.cutoff, d.pdb_id) == ("", None, "heavy", False, False, 8.0, [])
    a = p.parse_args(["--pdbdir", "o", "--data_dir", "d", "--split", "s.csv", "--suffix", "_R1", "--ref_suffixes", "_R1", "_R2", "_R3",
                      "--fit", "ca", "--no_pca", "--save"])
    assert (a.suffix, a.ref_suffixes, a.fit, a.no_pca, a.save) == ("_R1", ["_R1", "_R2", "_R3"], "ca", True, True)
    for bad in (["--fit", "all"], ["--plot"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--pdbdir", "o", "--data_dir", "d", "--split", "s.csv"] + bad)
    with pytest.raises(SystemExit):
        p.parse_args(["--data_dir", "d", "--split", "s.csv"])
    # the device calls -> the restatement
    monkeypatch.setattr(E, "analyze_ensemble", lambda traj, ref, aat, fit, cutoff, pca: R.analyze_ensemble(traj, ref, aat, fit, cutoff, pca))
    traj, ref, aat = R.analyze_case(L=8, T=16, F=16)
    from mdgen_amd.geometry import restype_order
    letters = {v: k for k, v in restype_order.items()}
    seq = "".join(letters[int(i)] for i in aat)
    out, data = tmp_path / "out", tmp_path / "data"
    out.mkdir()
    data.mkdir()
    split = tmp_path / "split.csv"
    split.write_text(f"name,seqres\npA,{seq}\npB,{seq}\npC,{seq}\npD,{seq}\npE,{seq}A\n")
    np.save(out / "pA.npy", traj)
    for s, part in (("_R1", ref[:10]), ("_R2", ref[10:])):
        np.save(data / f"pA{s}.npy", part)
    np.save(out / "pB.npy", traj)                                 # pB: one replica missing
    np.save(data / "pB_R1.npy", ref)
    np.save(data / "pC_R1.npy", ref)                              # pC: no sampled trajectory
    np.save(data / "pC_R2.npy", ref)
    np.save(out / "pD.npy", traj[:, :7])                          # pD: shapes disagree
    np.save(data / "pD_R1.npy", ref)
    np.save(data / "pD_R2.npy", ref)
    np.save(out / "pE.npy", traj)                                 # pE: the split's sequence is longer than the arrays
    np.save(data / "pE_R1.npy", ref)
    np.save(data / "pE_R2.npy", ref)
    common = ["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--ref_suffixes", "_R1", "_R2"]
    res = cli.main(common + ["--save"])
    cap = capsys.readouterr()
    assert list(res) == ["pA"] and "1 of 5 proteins analysed" in cap.out
    for name, why in (("pB", "pB_R2.npy"), ("pC", "neither"), ("pD", "shape"), ("pE", "shape")):
        line = [ln for ln in cap.err.splitlines() if ln.startswith(name + ": skipped")]
        assert len(line) == 1 and why in line[0], (name, cap.err)
    want = R.analyze_ensemble(traj, ref, aat)
    saved = pickle.load(open(out / "ensemble.pkl", "rb"))
    assert set(saved) == {"pA"} and set(saved["pA"]) == set(want)
    for key, v in want.items():
        assert isinstance(saved["pA"][key], (float, np.ndarray)) and np.array_equal(saved["pA"][key], v, equal_nan=True), key
    with pytest.raises(SystemExit, match="pZ"):
        cli.main(common + ["--pdb_id", "pZ"])
    with pytest.raises(SystemExit, match="cutoff"):
        cli.main(common + ["--cutoff", "-1"])
    one = cli.main(["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--suffix", "_R1", "--pdb_id", "pA", "--no_pca"])
    assert "pca_w2_ref" not in one["pA"] and np.array_equal(one["pA"]["ca_rmsf"], R.analyze_ensemble(traj, ref[:10], aat)["ca_rmsf"])


def test_sampling_clis_take_the_new_flags_and_default_to_off():
    from mdgen_amd import sim_inference, tps_inference, upsampling_inference
    s = sim_inference.build_parser().parse_args(["--data_dir", "d"])
    assert not s.superpose and not s.ensemble
    s = sim_inference.build_parser().parse_args(["--data_dir", "d", "--analyze", "--ensemble", "--superpose"])
    assert s.superpose and s.ensemble and s.analyze
    assert not tps_inference.build_parser().parse_args([]).superpose and tps_inference.build_parser().parse_args(["--superpose"]).superpose
    u = upsampling_inference.build_parser()
    assert not u.parse_args(["--data_dir", "d"]).superpose and u.parse_args(["--data_dir", "d", "--superpose"]).superpose


def test_host_half_imports_without_torch():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None; import numpy as np; import mdgen_amd.ensemble as E; "
            "print(E.jaccard([1, 0], [1, 1]), E.gaussian_w2(np.zeros((1, 3)), np.eye(3)[None], np.zeros((1, 3)), np.eye(3)[None])[2] < 1e-7)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "0.5 True", r.stderr
