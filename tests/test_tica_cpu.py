"""tICA without a device: the four entry points' bindings and refusals, `analysis.tica_solve` against tests/tica_ref.py and
against scipy's generalised eigensolver, rank-deficient inputs, the command lines' options -- and tica_ref.py, the NumPy
restatement the kernels of csrc/k_tica.hip are held against on the GPU, against double loops."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tica_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mdgen_traj_lagged_moments_workspace_bytes": ["n", "NF", "lag", "bytes"],
       "mdgen_traj_lagged_moments": ["n", "NF", "lag", "angles", "sx", "sy", "cxx", "cyy", "cxy", "workspace", "workspace_bytes",
                                     "stream"],
       "mdgen_traj_project": ["n", "NF", "d", "angles", "mean", "W", "out", "stream"],
       "mdgen_traj_series_acov_workspace_bytes": ["n", "NS", "K", "bytes"],
       "mdgen_traj_series_acov": ["n", "NS", "K", "x", "acov", "mean", "workspace", "workspace_bytes", "stream"],
       "mdgen_traj_histograms_xy": ["F", "NC", "values", "P", "pairs", "bins", "edges_x", "edges_y", "hist2", "dropped", "stream"]}


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
    """Every refusal is decided on the host, before any device call: the pointers (host memory here, holding a sentinel) are never
    dereferenced, and this runs where there is no device at all."""
    import mdgen_amd._lib as L
    buf = (ctypes.c_uint8 * 64)(*([0xA5] * 64))
    p = ctypes.addressof(buf)
    pairs = np.array([[0, 1]], np.int32)
    err = L.lib.mdgen_last_error
    mom, mom_ws = L.lib.mdgen_traj_lagged_moments, L.lib.mdgen_traj_lagged_moments_workspace_bytes
    proj, sac, sac_ws, hxy = (L.lib.mdgen_traj_project, L.lib.mdgen_traj_series_acov, L.lib.mdgen_traj_series_acov_workspace_bytes,
                              L.lib.mdgen_traj_histograms_xy)
    b = ctypes.c_size_t()
    big = 1 << 30
    # moments: lag = n, lag < 0, n < 1, NF = 65 refused; NF = 0 a no-op; null pointer; workspace
    for n, NF, lag in ((5, 1, 5), (5, 1, -1), (0, 1, 0), (5, 65, 1), (5, -1, 1)):
        assert mom(n, NF, lag, p, p, p, p, p, p, p, big, None) == -2, (n, NF, lag)
        assert mom_ws(n, NF, lag, ctypes.byref(b)) == -2
    assert b"NF must be in 0 .. 64" in err()
    assert mom(5, 1, 5, p, p, p, p, p, p, p, big, None) == -2 and b"lag must be in 0 .. n - 1" in err()
    assert mom(5, 1, 1, p, p, None, p, p, p, p, big, None) == -1 and b"null" in err()
    assert mom(5, 1, 1, p, p, p, p, p, p, p, 0, None) == -3
    assert mom(5, 0, 1, None, None, None, None, None, None, None, 0, None) == 0
    assert mom_ws(5, 1, 1, None) == -1 and mom_ws(5, 0, 1, ctypes.byref(b)) == 0 and b.value == 0
    # the sampler's size and the MD size: the features (n x 2 NF floats) and a few tens of MB of partial sums
    assert mom_ws(100000, 25, 1000, ctypes.byref(b)) == 0 and 100000 * 50 * 4 <= b.value < 1 << 27
    assert mom_ws(1000000, 25, 1000, ctypes.byref(b)) == 0 and 1000000 * 50 * 4 <= b.value < 1 << 28
    assert mom_ws(1000000, 64, 1000, ctypes.byref(b)) == 0 and b.value < 1 << 30
    # project: d = 0 and d = D + 1 refused
    for d in (0, 5, -1):
        assert proj(7, 2, d, p, p, p, p, None) == -2 and b"d must be in 1 .. 2 NF" in err()
    assert proj(7, 65, 1, p, p, p, p, None) == -2 and proj(0, 2, 1, p, p, p, p, None) == -2
    assert proj(7, 2, 4, p, p, None, p, None) == -1
    assert proj(7, 0, 1, None, None, None, None, None) == 0
    # series acov: K = n refused, as mdgen_traj_acov
    for n, K in ((0, 0), (5, 5), (5, -1), (1, 1)):
        assert sac(n, 1, K, p, p, p, p, big, None) == -2 and b"must be in" in err(), (n, K)
        assert sac_ws(n, 1, K, ctypes.byref(b)) == -2
    assert sac(5, 1, 4, p, p, p, p, 0, None) == -3
    assert sac(5, 1, 4, p, None, p, p, big, None) == -1
    assert sac(5, 0, 4, None, None, None, None, 0, None) == 0
    assert sac_ws(100000, 1, 1000, ctypes.byref(b)) == 0 and 100000 * 4 <= b.value < 1 << 24
    assert sac_ws(1000000, 1, 100000, ctypes.byref(b)) == 0 and b.value < 1 << 27
    # histograms_xy
    ok = lambda F=1, NC=2, P=1, pr=pairs, bins=50: hxy(F, NC, p, P, pr.ctypes.data, bins, p, p, p, p, None)  # noqa: E731
    assert ok(F=0) == -2 and ok(NC=0) == -2 and ok(bins=0) == -2 and ok(bins=129) == -2 and ok(P=-1) == -2
    assert ok(NC=1) == -2 and b"pairs[0][1] = 1" in err()
    assert ok(pr=np.array([[-1, 0]], np.int32)) == -2
    assert hxy(1, 2, p, 1, pairs.ctypes.data, 50, None, p, p, p, None) == -1
    assert hxy(1, 2, None, 0, None, 50, None, None, None, None, None) == 0
    assert bytes(buf) == b"\xa5" * 64


def test_python_refusals_come_before_the_device():
    """tica_fit and the *_into wrappers refuse bad shapes with ValueError before they look at the tensors' device: CPU tensors,
    which any launch would refuse with MdgenError, never get that far."""
    torch = pytest.importorskip("torch")
    from mdgen_amd import analysis as A
    ang = torch.zeros(12, 3)
    out = torch.full((64,), -7777.0, dtype=torch.float64)
    for lag in (11, 12, 13, -1):                      # n - lag < 2; lag = n; beyond
        with pytest.raises(ValueError, match="lag"):
            A.tica_fit(ang, lag)
    with pytest.raises(ValueError, match="torsions"):
        A.tica_fit(torch.zeros(12, 65), 1)
    with pytest.raises(ValueError, match="torsions"):
        A.tica_fit(torch.zeros(12, 0), 1)
    with pytest.raises(ValueError, match="lag must be in"):
        A.lagged_moments_into(ang, 12, out, out, out, out, out, torch.zeros(1 << 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="torsions"):
        A.lagged_moments_into(torch.zeros(12, 65), 1, out, out, out, out, out, torch.zeros(1 << 16, dtype=torch.uint8))
    o32 = torch.full((64,), -7777.0)
    for d in (0, 7):                                  # d = 0 and d = D + 1
        with pytest.raises(ValueError, match="expected"):
            A.project_into(ang, torch.zeros(6), torch.zeros(6, d), o32)
    model = A.TicaModel(1, np.zeros(6), np.ones(3), np.zeros((6, 3)), 2, 3)
    for d in (0, 4):
        with pytest.raises(ValueError, match="dim must be in"):
            A.tica_transform(model, ang.numpy(), d)
    assert (out == -7777.0).all() and (o32 == -7777.0).all()


def test_moments_restatement_equals_the_double_loop():
    ang = T.ou_angles(7, 2, 3)
    for lag in (0, 1, 3, 6):
        got, want = T.moments(ang, lag), T.moments_loop(ang, lag)
        for g, w in zip(got, want):
            assert np.abs(g - w).max() < 1e-14
        if lag == 0:
            assert np.array_equal(got[2], got[3]) and np.array_equal(got[2], got[4]) and np.array_equal(got[0], got[1])
    x = T.features32(ang)
    assert x.dtype == np.float32 and x.shape == (7, 4)
    assert np.array_equal(x[:, 0], np.cos(ang[:, 0].astype(np.float64)).astype(np.float32))      # cos first, then sin
    assert np.array_equal(x[:, 3], np.sin(ang[:, 1].astype(np.float64)).astype(np.float32))


def test_series_acov_restatement_equals_the_double_loop():
    x = 3.0 * T.ou_angles(9, 2, 5) + 0.4
    got, mean = T.series_acov(x, 8)
    assert np.abs(got - T.series_acov_loop(x, 8)).max() < 1e-13
    assert np.allclose(mean, x.astype(np.float64).mean(0), atol=1e-15)
    assert np.abs(T.series_acov(np.full((9, 1), 0.7), 8)[0] - 0.49).max() < 1e-14


def test_ou_angles():
    a = T.ou_angles(2000, 10, 7)
    assert a.dtype == np.float32 and a.shape == (2000, 10) and not a.flags.writeable
    assert (a > -np.pi).all() and (a <= float(np.float32(np.pi))).all()
    assert a is T.ou_angles(2000, 10, 7) and not np.array_equal(a, T.ou_angles(2000, 10, 8))


@pytest.mark.parametrize("case", T.EIG_CASES)
def test_tica_solve_against_the_restatement_and_scipy(case):
    from mdgen_amd.analysis import tica_solve
    la = pytest.importorskip("scipy.linalg")
    ang, m, mom, ref = T.eig_case(*case)
    model = tica_solve(m, *mom, lag=case[2])
    D = 2 * case[1]
    assert model.lag == case[2] and model.rank == ref["rank"] == D and model.dim == ref["dim"] and 2 <= model.dim < D
    assert model.W.shape == (D, D) and model.W.dtype == np.float64 and model.mean.shape == (D,)
    lam = model.eigenvalues
    assert (np.diff(lam) <= 0).all() and np.abs(lam - ref["eigenvalues"]).max() <= 1e-9
    assert np.abs(model.mean - ref["mean"]).max() <= 1e-15
    c0, ct = ref["C0"], ref["Ctau"]
    gl, gv = la.eigh(ct, c0)                                  # full rank: scipy's generalised problem applies; v' C0 v = 1
    gl, gv = gl[::-1], gv[:, ::-1]
    assert np.abs(lam - gl).max() <= 1e-9
    for c in range(model.dim):
        col = model.W[:, c]
        norm = np.linalg.norm(col)
        assert col[np.argmax(np.abs(col))] > 0
        assert np.abs(col - ref["W"][:, c]).max() <= 1e-6 * norm, c
        v = gv[:, c] * gl[c]
        v = v if v[np.argmax(np.abs(v))] > 0 else -v
        assert np.abs(col - v).max() <= 1e-6 * norm, c
    W = model.W
    assert np.abs(W.T @ c0 @ W - np.diag(lam ** 2)).max() <= 1e-9
    assert np.abs(W.T @ ct @ W - np.diag(lam ** 3)).max() <= 1e-9
    share = np.cumsum(lam ** 2) / np.sum(lam ** 2)
    assert share[model.dim - 1] >= 0.95 and (model.dim == 1 or share[model.dim - 2] < 0.95)
    d = model.as_dict()
    assert list(d) == ["lag", "mean", "eigenvalues", "W", "dim", "rank"] and type(d["dim"]) is int and type(d["W"]) is np.ndarray


def test_tica_solve_of_rank_deficient_features():
    from mdgen_amd.analysis import tica_solve
    base = T.ou_angles(3000, 5, 2)
    const = np.array(base)
    const[:, 2] = 0.7                                         # one torsion constant over all frames
    copy = np.array(base)
    copy[:, 4] = copy[:, 1]                                   # one column an exact copy of another
    for ang in (const, copy):
        mom = T.moments(ang, 5)
        model, ref = tica_solve(ang.shape[0] - 5, *mom, lag=5), T.solve(ang.shape[0] - 5, *mom)
        assert model.rank == ref["rank"] == 10 - 2 and model.W.shape == (10, 8) and 2 <= model.dim <= 8
        assert all(np.isfinite(x).all() for x in (model.mean, model.eigenvalues, model.W))
        assert np.abs(model.eigenvalues - ref["eigenvalues"]).max() <= 1e-9
        y = T.transform(ang, model.mean, model.W[:, :model.dim])
        assert np.isfinite(y).all()


def test_tica_solve_refuses_rank_below_two():
    from mdgen_amd.analysis import tica_solve
    ang = np.full((50, 3), 0.3, np.float32)                   # every feature constant: rank 0
    with pytest.raises(ValueError, match="rank"):
        tica_solve(45, *T.moments(ang, 5))
    ang = np.array(ang)
    ang[:, 0] = np.where(np.arange(50) % 2 == 0, 0.0, np.pi)  # cos +-1, sin 0 (to fp32 rounding of pi: below epsilon): rank 1
    with pytest.raises(ValueError, match="rank 1"):
        tica_solve(45, *T.moments(ang, 5))


def test_tica_solve_imports_without_torch():
    import subprocess
    code = ("import sys; sys.modules['torch'] = None\n"
            "import numpy as np\nfrom mdgen_amd.analysis import tica_solve, TicaModel, TICA_LAG\n"
            "g = np.random.default_rng(0); x = g.normal(size=(200, 4)); X, Y = x[:-3], x[3:]\n"
            "m = tica_solve(197, X.sum(0), Y.sum(0), X.T @ X, Y.T @ Y, X.T @ Y, lag=3)\n"
            "assert m.rank == 4 and TICA_LAG == 1000 and 'torch' not in [k for k, v in sys.modules.items() if v is not None]\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_options(tmp_path, capsys):
    from mdgen_amd import analyze_peptide_sim as cli
    from mdgen_amd import sim_inference
    nowhere = str(tmp_path / "nowhere")
    with pytest.raises(SystemExit) as e:                      # --tica does not lift the refusal: the MSM part is still absent
        cli.main(["--pdbdir", nowhere, "--data_dir", nowhere, "--split", nowhere + ".csv", "--tica"])
    assert e.value.code == 2 and "pyemma" in capsys.readouterr().err
    a = cli.build_parser().parse_args(["--pdbdir", "x", "--no_msm", "--tica", "--tica_lag", "5"])
    assert a.tica and a.tica_lag == 5 and a.no_msm
    a = cli.build_parser().parse_args(["--pdbdir", "x", "--no_msm"])
    assert not a.tica and a.tica_lag == 1000
    need = ["--data_dir", "x", "--out_dir", "y"]
    s = sim_inference.build_parser().parse_known_args(need + ["--analyze", "--tica", "--tica_lag", "1"])[0]
    assert s.analyze and s.tica and s.tica_lag == 1
    s = sim_inference.build_parser().parse_known_args(need)[0]
    assert not s.tica and s.tica_lag == 1000
