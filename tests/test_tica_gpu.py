"""csrc/k_tica.hip on the GPU against tests/tica_ref.py (gates: its docstring).

Every output buffer is pre-filled with a sentinel and has a guard region of the sentinel behind it; the guards must be intact, no
sentinel may be left where an output belongs, and a second call gives the same bits.  Histograms are compared with
np.histogram / np.histogram2d of the values widened to fp64, exactly."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import analysis_ref as R  # noqa: E402
import tica_ref as T  # noqa: E402

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


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype)).to(_cuda())   # (a copy: the cases are read-only)


# ---- lagged moments -------------------------------------------------------------------------------------------------
def run_moments(angles, lag):
    from mdgen_amd.analysis import lagged_moments_into, lagged_moments_workspace_bytes
    n, NF = angles.shape
    D = 2 * NF
    ws = torch.empty(lagged_moments_workspace_bytes(n, NF, lag), dtype=torch.uint8, device=_cuda())
    sizes = (D, D, D * D, D * D, D * D)
    bufs = [_guarded(k, torch.float64, SENT_F) for k in sizes]
    lagged_moments_into(_dev(angles), lag, *[v for _, v in bufs], ws)
    torch.cuda.synchronize()
    for (b, _), k in zip(bufs, sizes):
        _guard_ok(b, k, SENT_F)
    out = [v.cpu().numpy() for _, v in bufs]
    assert not any((o == SENT_F).any() for o in out), "an output was not written"
    return [out[0], out[1]] + [o.reshape(D, D) for o in out[2:]]


MOMENT_CASES = [(1, 0, 1, False), (2, 1, 1, False), (2, 0, 3, False), (65, 1, 3, False), (65, 64, 22, False), (257, 7, 64, False),
                (4099, 1000, 22, False), (4099, 1000, 22, True), (100003, 1000, 8, False)]


@pytest.mark.parametrize("n,lag,NF,constant", MOMENT_CASES)
def test_lagged_moments(n, lag, NF, constant):
    ang = T.ou_angles(n, NF, n + NF)
    if constant:
        ang = np.array(ang)
        ang[:, 3] = 0.7                                       # a constant column: its features have no variance
    m = n - lag
    got = run_moments(ang, lag)
    want, low = T.moments(ang, lag), T.moments32(ang, lag)
    for name, g, w, lo in zip(("sx", "sy", "cxx", "cyy", "cxy"), got, want, low):
        floor = np.abs(lo.astype(np.float64) - w).max() / m
        err = np.abs(g - w).max() / m
        print(f"moments n {n} lag {lag} NF {NF} {name}: error {err:.3e}, gate {T.gate(floor):.3e}")
        assert err <= T.gate(floor), (name, err, T.gate(floor))
    if lag == 0:
        assert np.array_equal(got[2], got[3]) and np.array_equal(got[2], got[4]) and np.array_equal(got[0], got[1])
    assert np.array_equal(got[2], got[2].T) and np.array_equal(got[3], got[3].T)      # (a product commutes to the bit)
    again = run_moments(ang, lag)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "a second call gave other bits"


# ---- projection -----------------------------------------------------------------------------------------------------
def run_project(angles, mean, W):
    from mdgen_amd.analysis import project_into
    n, d = angles.shape[0], W.shape[1]
    buf, out = _guarded(n * d, torch.float32, SENT_F)
    project_into(_dev(angles), _dev(mean), _dev(W), out)
    torch.cuda.synchronize()
    _guard_ok(buf, n * d, SENT_F)
    got = out.cpu().numpy().reshape(n, d)
    assert not (got == SENT_F).any(), "an output was not written"
    return got


@pytest.mark.parametrize("NF,d", [(1, 1), (1, 2), (22, 2), (22, 44), (64, 7)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_project(n, NF, d):
    ang = T.ou_angles(4099, NF, 100 + NF)[:n]
    g = np.random.default_rng(n + NF + d)
    mean = (0.5 * g.normal(size=2 * NF)).astype(np.float32)
    W = g.normal(size=(2 * NF, d)).astype(np.float32)
    got = run_project(ang, mean, W)
    want = T.transform(ang, mean, W)
    floor = np.abs(T.transform32(ang, mean, W).astype(np.float64) - want).max()
    gate = T.gate(floor, np.abs(want).max())
    err = np.abs(got - want).max()
    print(f"project n {n} NF {NF} d {d}: error {err:.3e}, gate {gate:.3e}")
    assert err <= gate, (err, gate)
    assert np.array_equal(got, run_project(ang, mean, W)), "a second call gave other bits"


def test_project_refusal_leaves_the_output_alone():
    from mdgen_amd._lib import MdgenError, launch, lib, ptr
    dev = _cuda()
    buf, out = _guarded(64, torch.float32, SENT_F)
    ang, mean, W = torch.zeros(8, 2, device=dev), torch.zeros(4, device=dev), torch.zeros(4, 5, device=dev)
    for d in (0, 5):
        with pytest.raises(MdgenError, match="d must be in 1 .. 2 NF"):
            launch(lib.mdgen_traj_project, ang, 8, 2, d, ptr(ang), ptr(mean), ptr(W), ptr(out))
    torch.cuda.synchronize()
    assert (buf == SENT_F).all().item()


# ---- autocovariance of a series -------------------------------------------------------------------------------------
def run_series_acov(x, K):
    from mdgen_amd.analysis import series_acov_into, series_acov_workspace_bytes
    n, NS = x.shape
    ws = torch.empty(series_acov_workspace_bytes(n, NS, K), dtype=torch.uint8, device=_cuda())
    na = NS * (K + 1)
    ba, acov = _guarded(na, torch.float64, SENT_F)
    bm, mean = _guarded(NS, torch.float64, SENT_F)
    series_acov_into(_dev(x), K, acov, mean, ws)
    torch.cuda.synchronize()
    _guard_ok(ba, na, SENT_F)
    _guard_ok(bm, NS, SENT_F)
    out = acov.cpu().numpy().reshape(NS, K + 1), mean.cpu().numpy()
    assert not any((o == SENT_F).any() for o in out), "an output was not written"
    return out


SERIES_CASES = sorted({(n, K) for n, K, _ in [(1, 0, 1), (1, 0, 23), (2, 1, 1), (2, 1, 23), (65, 64, 1), (65, 64, 23), (1001, 1000, 1),
                                              (1001, 1000, 23), (4097, 1000, 1), (4097, 1000, 23), (100003, 1000, 4)]})   # ACOV_CASES' (n, K)


def _series(n, NS):
    return (3.0 * T.ou_angles(n, NS, n + NS) + (0.5 + 0.25 * np.arange(NS))).astype(np.float32)


@pytest.mark.parametrize("NS", [1, 3])
@pytest.mark.parametrize("n,K", SERIES_CASES)
def test_series_acov(n, K, NS):
    x = _series(n, NS)
    got, mean = run_series_acov(x, K)
    want, wmean = T.series_acov(x, K)
    lags = None if n * NS <= 5000 else sorted(set(range(0, K + 1, 37)) | {1, K - 1, K})   # (the floor: np.dot per lag and series)
    gate = T.gate(T.series_acov_floor(x, K, lags), np.abs(want).max())
    err = np.abs(got - want).max()
    print(f"series acov n {n} K {K} NS {NS}: error {err:.3e}, gate {gate:.3e}")
    assert err <= gate, (err, gate)
    assert np.abs(mean - wmean).max() <= T.gate(np.abs(x.mean(0, dtype=np.float32) - wmean).max(), np.abs(wmean).max())
    again = run_series_acov(x, K)
    assert np.array_equal(got, again[0]) and np.array_equal(mean, again[1]), "a second call gave other bits"


def test_series_acov_of_a_constant_series():
    c = np.float32(1.7)
    x = np.full((4097, 2), c, np.float32)
    got, mean = run_series_acov(x, 1000)
    c2 = float(c) ** 2
    gate = T.gate(T.series_acov_floor(x, 1000, range(0, 1001, 100)), c2)
    assert np.abs(got - c2).max() <= gate, (np.abs(got - c2).max(), gate)
    assert np.abs(mean - float(c)).max() <= T.EPS32 * float(c)


def test_series_acov_refuses_K_equal_n():
    from mdgen_amd._lib import MdgenError
    from mdgen_amd.analysis import series_acov_into
    dev = _cuda()
    ba, acov = _guarded(2 * 66, torch.float64, SENT_F)
    bm, mean = _guarded(2, torch.float64, SENT_F)
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=dev)
    with pytest.raises(MdgenError, match="K must be in 0 .. n - 1"):
        series_acov_into(torch.zeros(65, 2, device=dev), 65, acov, mean, ws)
    torch.cuda.synchronize()
    assert (ba == SENT_F).all().item() and (bm == SENT_F).all().item() and (ws == 0x5A).all().item()


# ---- 2-D histograms with their own edges ----------------------------------------------------------------------------
def run_hist_xy(values, pairs, bins, ranges):
    from mdgen_amd.analysis import histograms_xy_into, range_edges
    dev = _cuda()
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    ex = np.stack([range_edges(*r[0], bins) for r in ranges])
    ey = np.stack([range_edges(*r[1], bins) for r in ranges])
    b2, h2 = _guarded(P * bins * bins, torch.int64, SENT_I)
    bd, dr = _guarded(P, torch.int64, SENT_I)
    histograms_xy_into(_dev(values), pairs, bins, torch.from_numpy(ex).to(dev), torch.from_numpy(ey).to(dev), h2, dr)
    torch.cuda.synchronize()
    _guard_ok(b2, P * bins * bins, SENT_I)
    _guard_ok(bd, P, SENT_I)
    return h2.cpu().numpy().reshape(P, bins, bins), dr.cpu().numpy()


def check_hist_xy(values, pairs, bins, ranges):
    v64 = np.asarray(values, np.float32).astype(np.float64)
    h2, dr = run_hist_xy(values, pairs, bins, ranges)
    for j, ((cx, cy), r) in enumerate(zip(pairs, ranges)):
        want = np.histogram2d(v64[:, cx], v64[:, cy], bins=bins, range=r)[0].astype(np.int64)
        assert np.array_equal(h2[j], want), j
        assert dr[j] == len(v64) - want.sum(), j
    again = run_hist_xy(values, pairs, bins, ranges)
    assert np.array_equal(h2, again[0]) and np.array_equal(dr, again[1])
    return h2, dr


@pytest.mark.parametrize("P", [1, 2, 65])
@pytest.mark.parametrize("F", [1, 1000, 100003])
def test_histograms_xy_over_the_data_range(F, P):
    """Ranges: every column's own minimum and maximum, so the largest value lands in the last bin and nothing is dropped (F = 1:
    every range is degenerate)."""
    v = (T.ou_angles(F, 4, F) * np.array([1.0, 5.0, 0.01, 300.0]) + np.array([0.0, -7.0, 2.0, 1e3])).astype(np.float32)
    pairs = [(i % 4, (i * 3 + 1) % 4) for i in range(P)]      # 64 pairs a launch
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    ranges = [((lo[a], hi[a]), (lo[b], hi[b])) for a, b in pairs]
    h2, dr = check_hist_xy(v, pairs, R.BINS_2D, ranges)
    assert (dr == 0).all() and (h2.sum((1, 2)) == F).all()
    if F > 1:
        for j, (a, b) in enumerate(pairs):
            assert h2[j, -1].sum() >= 1 and h2[j, :, -1].sum() >= 1      # the maxima: in the last bins


def test_histograms_xy_at_the_edges():
    from mdgen_amd.analysis import range_edges
    rx, ry = (-1.3, 2.9), (0.1, 7.7)
    cols = []
    for r in (rx, ry):
        v = []
        for e in range_edges(*r, R.BINS_2D):
            x = np.float32(e)
            v += [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
        cols.append(np.array(v, np.float32))
    v = np.stack([cols[0], np.roll(cols[1][::-1], 7)], 1)
    h2, dr = check_hist_xy(v, [(0, 1), (1, 0)], R.BINS_2D, [(rx, ry), (ry, rx)])
    assert dr[0] == dr[1] >= 2 and np.array_equal(h2[0], h2[1].T)       # the neighbours beyond the outer edges are in no bin
    check_hist_xy(v, [(0, 1)], 7, [(rx, ry)])


def test_histograms_xy_of_a_degenerate_range():
    v = np.stack([np.full(1000, 0.25, np.float32), T.ou_angles(1000, 1, 3)[:, 0]], 1)
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    h2, dr = check_hist_xy(v, [(0, 1), (1, 0)], R.BINS_2D, [((lo[0], hi[0]), (lo[1], hi[1])), ((lo[1], hi[1]), (lo[0], hi[0]))])
    assert dr.sum() == 0 and (h2[0].sum(1) > 0).sum() == 1 and h2[0].sum() == 1000


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_analyze_with_tica_against_the_restatement():
    from mdgen_amd import analysis as A
    dev = _cuda()
    aatype = R.aatype_of("FLRH")
    traj, ref = R.peptide(2000, aatype, seed=21, walk=0.15), R.peptide(5000, aatype, seed=22, walk=0.15)
    got = A.analyze(torch.from_numpy(traj).to(dev), ref, aatype, nlag=200, ref_nlag=200, tica=True, tica_lag=10)
    assert list(got) == ["features", "JSD", "our_decorrelation", "md_decorrelation", "tica_model"]
    assert list(got["JSD"])[-2:] == ["TICA-0", "TICA-0,1"] and len(got["JSD"]) == 16 + 2 + 2
    assert list(got["our_decorrelation"])[-1] == "tica" and list(got["md_decorrelation"])[-1] == "tica"
    model = got["tica_model"]
    assert list(model) == ["lag", "mean", "eigenvalues", "W", "dim", "rank"] and model["lag"] == 10
    assert all(type(model[k]) is np.ndarray and model[k].dtype == np.float64 for k in ("mean", "eigenvalues", "W"))
    assert type(model["dim"]) is int and type(model["rank"]) is int and model["W"].shape == (32, model["rank"])
    pickle.loads(pickle.dumps(got))
    # each stage on the previous stage's device output.  Moments -> solver:
    a_traj, a_ref = A.featurize(torch.from_numpy(traj).to(dev), aatype), A.featurize(torch.from_numpy(ref).to(dev), aatype)
    mom = [p.cpu().numpy() for p in A.lagged_moments(a_ref, 10)]
    want = T.solve(5000 - 10, *mom)
    assert model["rank"] == want["rank"] and model["dim"] == want["dim"]
    assert np.abs(model["eigenvalues"] - want["eigenvalues"]).max() <= 1e-9
    # ... projected values -> histograms and JSDs:
    d = max(model["dim"], 2)
    y_ref, y_traj = (A.tica_transform(model, a, d).cpu().numpy().astype(np.float64) for a in (a_ref, a_traj))
    lo = np.minimum(y_ref[:, :2].min(0), y_traj[:, :2].min(0))
    hi = np.maximum(y_ref[:, :2].max(0), y_traj[:, :2].max(0))
    r1, t1 = (np.histogram(y[:, 0], range=(lo[0], hi[0]), bins=100)[0] for y in (y_ref, y_traj))
    rng = ((lo[0], hi[0]), (lo[1], hi[1]))
    r2, t2 = (np.histogram2d(y[:, 0], y[:, 1], range=rng, bins=50)[0] for y in (y_ref, y_traj))
    for y, w1, w2 in ((y_ref, r1, r2), (y_traj, t1, t2)):
        yd = torch.from_numpy(y.astype(np.float32)).to(dev)
        assert np.array_equal(A._hist1d_range(yd, 0, lo[0], hi[0], 100), w1)
        h2, dr = A.histogram2d_xy(yd, [(0, 1)], 50, [rng])
        assert np.array_equal(h2[0], w2) and dr[0] == 0 and w1.sum() == w2.sum() == len(y)
    assert abs(got["JSD"]["TICA-0"] - A.jsd(r1, t1)) <= 1e-12 and abs(got["JSD"]["TICA-0,1"] - A.jsd(r2, t2)) <= 1e-12
    assert 0 < got["JSD"]["TICA-0"] < 0.84 and 0 < got["JSD"]["TICA-0,1"] < 0.84
    # ... component 0 -> the 'tica' curves:
    for key, y in (("our_decorrelation", y_traj), ("md_decorrelation", y_ref)):
        x = y[:, :1].astype(np.float32)
        wantc = T.series_acov(x, 200)[0][0]
        gate = T.gate(T.series_acov_floor(x, 200, range(0, 201, 20)), np.abs(wantc).max())
        g = got[key]["tica"]
        assert g.dtype == np.float32 and g.shape == (201,)
        assert np.abs(g.astype(np.float64) - wantc).max() <= gate, key
    # tica=False: the parent's result, key for key -- and the same entries inside the tica=True result
    plain = A.analyze(torch.from_numpy(traj).to(dev), ref, aatype, nlag=200, ref_nlag=200, tica=False)
    default = A.analyze(torch.from_numpy(traj).to(dev), ref, aatype, nlag=200, ref_nlag=200)
    assert list(plain) == list(default) == ["features", "JSD", "our_decorrelation", "md_decorrelation"]
    assert len(plain["JSD"]) == 16 + 2 and "tica" not in plain["our_decorrelation"]
    for other in (default, got):
        assert plain["features"] == other["features"]
        assert all(plain["JSD"][k] == other["JSD"][k] for k in plain["JSD"])
        assert list(plain["JSD"]) == list(other["JSD"])[:18]
        for key in ("our_decorrelation", "md_decorrelation"):
            assert all(np.array_equal(plain[key][lab], other[key][lab], equal_nan=True) for lab in plain["features"])


def _sim_inputs(tmp_path, names):
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import restype_order
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
    return data, split


def test_sim_inference_analyze_tica(tmp_path, capsys):
    """sim_inference --synthetic --analyze --tica at test_sim_inference_analyze's sizes (2 peptides, 50 frames, 3-frame MD files).
    --tica_lag 1: two lagged pairs, rank at most 2 -- it runs through, and a peptide whose tICA is refused is named on stderr and
    keeps its torsion entries.  --tica_lag 2: one lagged pair; every peptide is refused, named, and keeps its torsion entries."""
    from mdgen_amd import sim_inference as cli
    from mdgen_amd.analysis import analyze
    from mdgen_amd.geometry import restype_order
    dev = _cuda()
    names = {"FLRH": "FLRH", "AWKD": "AWKD"}
    data, split = _sim_inputs(tmp_path, names)
    common = ["--synthetic", "--data_dir", str(data), "--split", str(split), "--num_frames", "50", "--num_rollouts", "2",
              "--num_steps", "2", "--batch", "2", "--npy", "--analyze", "--tica"]
    for lag in (1, 2):
        out = tmp_path / f"out{lag}"
        capsys.readouterr()
        res = cli.main(common + ["--out_dir", str(out), "--tica_lag", str(lag)])
        err = capsys.readouterr().err
        assert res["names"] == list(names)
        got = pickle.load(open(out / "analysis.pkl", "rb"))
        assert list(got) == list(names)
        for n, sq in names.items():
            aat = np.array([restype_order[c] for c in sq])
            want = analyze(torch.from_numpy(np.load(out / f"{n}.npy")).to(dev), np.load(data / f"{n}.npy"), aat)
            assert got[n]["features"] == want["features"] and list(got[n]["JSD"])[:len(want["JSD"])] == list(want["JSD"])
            for lab in want["features"]:
                assert np.array_equal(got[n]["our_decorrelation"][lab], want["our_decorrelation"][lab], equal_nan=True)
            refused = "tica_model" not in got[n]
            assert refused == (f"{n}: no tICA entries" in err), (n, err)
            if refused:
                assert list(got[n]) == list(want) and list(got[n]["JSD"]) == list(want["JSD"])
            else:
                assert lag == 1 and got[n]["tica_model"]["rank"] == 2 and got[n]["tica_model"]["lag"] == 1
                assert list(got[n]["JSD"])[-2:] == ["TICA-0", "TICA-0,1"] and np.isfinite(got[n]["JSD"]["TICA-0"])
                assert got[n]["our_decorrelation"]["tica"].shape == (100,) and got[n]["md_decorrelation"]["tica"].shape == (3,)
        if lag == 2:
            assert all("tica_model" not in got[n] for n in names) and "needs at least lag + 2 frames" in err


def test_cli_analyze_peptide_sim_tica(tmp_path):
    """analyze_peptide_sim --no_msm --tica --tica_lag 5 --save on test_cli_analyze_peptide_sim's two peptides: the pickle holds
    analyze(..., tica=True, tica_lag=5) of what was read."""
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
    got = cli.main(["--pdbdir", str(out), "--data_dir", str(data), "--split", str(split), "--no_msm", "--tica", "--tica_lag", "5",
                    "--save", "--truncate", "250"])
    saved = pickle.load(open(out / "out.pkl", "rb"))
    assert list(got) == list(saved) == ["pA", "pB"]
    read = {"pA": trajs["pA"], "pB": pdb_to_atom14(str(out / "pB.pdb"), R.aatype_of("AWKD"))}
    for n, sq in names.items():
        want = analyze(torch.from_numpy(read[n][:250]).to(dev), np.load(data / f"{n}.npy"), R.aatype_of(sq), tica=True, tica_lag=5)
        assert list(saved[n]) == list(want) == ["features", "JSD", "our_decorrelation", "md_decorrelation", "tica_model"]
        assert saved[n]["features"] == want["features"] and saved[n]["JSD"] == want["JSD"]
        assert list(saved[n]["JSD"])[-2:] == ["TICA-0", "TICA-0,1"]
        for key in ("our_decorrelation", "md_decorrelation"):
            assert list(saved[n][key]) == want["features"] + ["tica"]
            assert all(np.array_equal(saved[n][key][lab], want[key][lab], equal_nan=True) for lab in want[key])
        assert saved[n]["our_decorrelation"]["tica"].shape == (250,) and saved[n]["md_decorrelation"]["tica"].shape == (400,)
        for k in ("mean", "eigenvalues", "W"):
            assert np.array_equal(saved[n]["tica_model"][k], want["tica_model"][k])
        assert saved[n]["tica_model"]["lag"] == 5 and saved[n]["tica_model"]["dim"] == want["tica_model"]["dim"]
