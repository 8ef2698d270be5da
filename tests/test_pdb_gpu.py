"""mdgen_pdb_format on the GPU (csrc/k_pdb.hip) against frames_to_pdb_string on the same float32 array: equality of bytes.

Every call gets a text buffer pre-filled with 0xFF and 64 guard bytes of 0xFF behind `text` and behind `offsets`; the guards must
be intact, no 0xFF may appear inside text[:total], and `offsets` must equal the cumulative lengths of the host writer's frames.
The arrays are those of tests/pdb_ref.py, which tests/test_pdb_device_cpu.py runs through the NumPy restatement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pdb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64


def _cuda():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda:0")


def run_kernels(atom14, aatype, model_base=0, capacity=None):
    """One mdgen_pdb_format call -> (text buffer as numpy uint8 [capacity], offsets [M + 1], status [2]); checks the guards."""
    from mdgen_amd.pdb import sequence_inputs, format_frames_device, frame_capacity
    dev = _cuda()
    aatype = np.asarray(aatype, np.int64)
    M = atom14.shape[0]
    cap = M * frame_capacity(aatype) if capacity is None else capacity
    tbuf = torch.full((cap + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    obuf = torch.full((M + 1 + GUARD // 8,), -1, dtype=torch.int64, device=dev)   # (-1: eight bytes of 0xFF)
    status = torch.full((2,), -1, dtype=torch.int64, device=dev)
    format_frames_device(torch.from_numpy(np.ascontiguousarray(atom14, np.float32)).to(dev), sequence_inputs(aatype, dev),
                         model_base, obuf[:M + 1], tbuf[:cap], status)
    torch.cuda.synchronize()
    t, o = tbuf.cpu().numpy(), obuf.cpu().numpy()
    assert (t[cap:] == 0xFF).all(), "guard behind text overwritten"
    assert (o[M + 1:] == -1).all(), "guard behind offsets overwritten"
    return t[:cap], o[:M + 1], status.cpu().numpy()


def check(atom14, aatype, model_base=0):
    want, want_off = R.host_text(atom14, aatype, model_base)
    text, off, status = run_kernels(atom14, aatype, model_base)
    assert status[0] == 0 and status[1] == len(want)
    assert np.array_equal(off, want_off)
    total = int(off[-1])
    assert not (text[:total] == 0xFF).any(), "a byte of the text was not written"
    assert (text[total:] == 0xFF).all(), "bytes behind the text were written"
    got = text[:total].tobytes()
    if got != want:   # name the first differing line instead of printing two trajectories
        g, w = got.split(b"\n"), want.split(b"\n")
        i = next(i for i in range(min(len(g), len(w))) if g[i] != w[i])
        raise AssertionError(f"line {i}: got {g[i]!r}, want {w[i]!r}")
    return got


def test_rounding():
    text = check(*R.rounding_case()).decode()
    assert "   0.062" in text and "   0.188" in text and "  -0.000" in text and "   0.000   1.000   1.000" in text


def test_presence():
    check(*R.presence_case())


def test_residue_types():
    for a, aatype in R.types_cases():
        check(a, aatype)


def test_model_digits():
    gly = np.array([R.GLY])
    check(R.plausible(1001, 1, seed=5), gly)
    check(R.plausible(4, 1, seed=6), gly, model_base=9998)


@pytest.mark.parametrize("L", [1, 2, 7, 19, 33, 64, 65, 256])
@pytest.mark.parametrize("M", [1, 3])
def test_launch_edges(M, L):
    check(*R.launch_edge_case(M, L))


def test_chunking_through_atom14_to_pdb(tmp_path):
    from mdgen_amd.pdb import atom14_to_pdb, frames_to_pdb_string
    a, aatype = R.plausible(25, 3, seed=7), np.array([R.SER, R.TRP, R.GLY])
    a[11, 1, 3] = 0
    want = frames_to_pdb_string(a, aatype).encode()
    dev_a = torch.from_numpy(a).to(_cuda())
    for chunk in (1, 7, 4096):
        p = tmp_path / f"c{chunk}.pdb"
        atom14_to_pdb(dev_a, aatype, p, chunk=chunk)
        assert open(p, "rb").read() == want, chunk
    atom14_to_pdb(dev_a, torch.from_numpy(aatype).to(_cuda()), tmp_path / "t.pdb")   # aatype as a device tensor, default chunk
    assert open(tmp_path / "t.pdb", "rb").read() == want


@pytest.mark.parametrize("name", list(R.REFUSED))
def test_refusal_and_fallback(name, tmp_path):
    from mdgen_amd.pdb import atom14_to_pdb, frames_to_pdb_string
    a, aatype = R.refusal_case(name)
    text, off, status = run_kernels(a, aatype)
    assert status[0] >= 1
    assert (text == 0xFF).all(), "the format pass wrote although a field overflows"
    atom14_to_pdb(torch.from_numpy(a).to(_cuda()), aatype, tmp_path / "x.pdb")
    assert open(tmp_path / "x.pdb", "rb").read() == frames_to_pdb_string(a, aatype).encode()


def test_capacity_one_byte_short():
    a, aatype = R.presence_case()
    want, _ = R.host_text(a, aatype)
    text, off, status = run_kernels(a, aatype, capacity=len(want) - 1)
    assert status[0] == 0 and status[1] == len(want) == off[-1]
    assert (text == 0xFF).all()
    text, off, status = run_kernels(a, aatype, capacity=len(want))   # ... and exactly enough is enough
    assert text.tobytes() == want


def _peptide_files(tmp_path, names, frames_of):
    data = tmp_path / "data"
    data.mkdir()
    for n, sq in names.items():
        np.save(data / frames_of[0].format(n=n), frames_of[1](sq))
    split = tmp_path / "split.csv"
    split.write_text("name,seqres\n" + "".join(f"{n},{s}\n" for n, s in names.items()))
    return data, split


def _assert_pdbs_match_npys(out, names):
    from mdgen_amd.geometry import restype_order
    from mdgen_amd.pdb import frames_to_pdb_string
    for n, sq in names.items():
        arr = np.load(out / f"{n}.npy")
        assert np.isfinite(arr).all()
        want = frames_to_pdb_string(arr, np.array([restype_order[c] for c in sq]))
        assert open(out / f"{n}.pdb").read() == want, n


def test_cli_sim_inference(tmp_path):
    """sim_inference --synthetic --npy, B 2 x T 8 x L 4, 2 rollouts: each .pdb (written from the device tensor) equals
    frames_to_pdb_string of its .npy."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import restype_order
    from mdgen_amd import sim_inference as cli
    _cuda()
    names = {"FLRH": "FLRH", "AWKD": "AWKD"}
    gen = torch.Generator().manual_seed(5)

    def first_frames(sq):
        seqres = torch.tensor([restype_order[ch] for ch in sq])
        q = torch.randn(1, 3, 4, 4, generator=gen)
        tr = torch.cumsum(2.2 * torch.randn(1, 3, 4, 3, generator=gen), 2)
        ang = torch.randn(1, 3, 4, 7, 2, generator=gen)
        return O.frames_torsions_to_atom14(O.quat_to_rot(q / q.norm(dim=-1, keepdim=True)), tr, ang / ang.norm(dim=-1, keepdim=True),
                                           seqres[None, None].expand(1, 3, 4))[0].numpy().astype(np.float16)
    data, split = _peptide_files(tmp_path, names, ("{n}.npy", first_frames))
    out = tmp_path / "out"
    torch.manual_seed(1234)
    res = cli.main(["--synthetic", "--data_dir", str(data), "--split", str(split), "--out_dir", str(out), "--num_frames", "8",
                    "--num_rollouts", "2", "--num_steps", "2", "--batch", "2", "--npy"])
    assert res["names"] == list(names) and res["frames"] == 2 * 2 * 8
    assert np.load(out / "FLRH.npy").shape == (16, 4, 14, 3)
    _assert_pdbs_match_npys(out, names)


def test_cli_upsampling_inference(tmp_path):
    """upsampling_inference --synthetic --npy on one window of three key frames (T = 12, cond_interval 4), one peptide."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import restype_order
    from mdgen_amd.upsampling_inference import main
    _cuda()
    names = {"pA": "FLRH"}
    gen = torch.Generator().manual_seed(6)

    def key_frames(sq):
        seqres = torch.tensor([restype_order[ch] for ch in sq])
        q = torch.randn(1, 3, 4, 4, generator=gen)
        tr = torch.cumsum(2.2 * torch.randn(1, 3, 4, 3, generator=gen), 2)
        ang = torch.randn(1, 3, 4, 7, 2, generator=gen)
        return O.frames_torsions_to_atom14(O.quat_to_rot(q / q.norm(dim=-1, keepdim=True)), tr, ang / ang.norm(dim=-1, keepdim=True),
                                           seqres[None, None].expand(1, 3, 4))[0].numpy().astype(np.float32)
    data, split = _peptide_files(tmp_path, names, ("{n}_i100.npy", key_frames))
    out = tmp_path / "out"
    res = main(["--synthetic", "--num_frames", "12", "--cond_interval", "4", "--batch_size", "1", "--num_steps", "2", "--npy",
                "--data_dir", str(data), "--split", str(split), "--out_dir", str(out)])
    assert res["names"] == ["pA"] and res["frames"] == 12
    _assert_pdbs_match_npys(out, names)
