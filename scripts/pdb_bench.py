"""Frames/s of writing a sampled trajectory as multi-model PDB text: the host formatter
(`frames_to_pdb_string`, one Python string per atom) beside the device path of `atom14_to_pdb` (`mdgen_pdb_format`,
csrc/k_pdb.hip), the latter taken apart: kernels only, kernels + copy to pinned memory, kernels + copy + file write.  Shapes:
`headline` B 16 x M 10 x 1000 x L 4 (one `sim_inference --batch 16 --num_rollouts 10` group: 16 files) and `atlas`
B 1 x M 250 x L 256; plausible coordinates, every atom of the sequence present.  One JSON line per (shape, leg).

    python scripts/pdb_bench.py [--shape headline|atlas] [--leg host|kernel|copy|file] [--reps 3] [--host-frames 1000]
    python scripts/pdb_bench.py --leg cli [--writer device|host] [--host-module FILE]

`--leg cli`: the wall clock of a `sim_inference --synthetic --batch 16 --num_rollouts 10` group in-process, sampling and
writing apart, on 32 generated tetrapeptides: two groups, the first pays the graph capture.  `--writer host` hands the writer the host copy of the array, as the drivers did
before the device path existed; `--host-module FILE` takes `frames_to_pdb_string` of the host legs from that file (another
revision's pdb.py) instead of this tree's.  As a job, run one leg per process, each under its own `timeout`.
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"headline": (16, 10 * 1000, 4), "atlas": (1, 250, 256)}


def host_formatter(path):
    if path is None:
        from mdgen_amd.pdb import frames_to_pdb_string
        return frames_to_pdb_string
    spec = importlib.util.spec_from_file_location("pdb_other", path)
    mod = importlib.util.module_from_spec(spec)
    mod.__file__ = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mdgen_amd", "pdb.py")   # (its tables)
    spec.loader.exec_module(mod)
    return mod.frames_to_pdb_string


def trajectory(B, M, L_, dev):
    """A random walk of residue centres 3.8 A apart with atoms within 2.5 A of them: coordinates of a peptide's size."""
    g = torch.Generator().manual_seed(0)
    centre = torch.cumsum(3.8 * torch.nn.functional.normalize(torch.randn(B, 1, L_, 1, 3, generator=g), dim=-1), 2)
    a = centre + 0.3 * torch.randn(B, M, 1, 1, 3, generator=g).cumsum(1) + 1.2 * torch.randn(B, M, L_, 14, 3, generator=g)
    return a.to(dev), (np.arange(L_) * 7 + 3) % 20


def timed(fn, reps):
    fn()   # warm-up: allocations, templates, pinned buffer
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def leg(shape, which, a):
    from mdgen_amd.pdb import CHUNK_FRAMES, _format_device, atom14_to_pdb
    B, M, L_ = SHAPES[shape]
    dev = torch.device("cuda")
    out = {"shape": shape, "B": B, "M": M, "L": L_, "leg": which}
    if which == "host":
        fmt = host_formatter(a.host_module)
        atom14, aatype = trajectory(1, min(M, a.host_frames), L_, "cpu")
        arr = atom14[0].numpy()
        t0 = time.perf_counter()
        text = fmt(arr, aatype)
        dt = time.perf_counter() - t0
        out.update(frames=arr.shape[0], seconds=dt, frames_per_s=arr.shape[0] / dt, bytes_per_frame=len(text) / arr.shape[0],
                   formatter=a.host_module or "this tree")
        return out
    atom14, aatype = trajectory(B, M, L_, dev)
    aat = np.asarray(aatype, np.int64)
    if which == "kernel":
        dt = timed(lambda: [_format_device(atom14[b], aat, CHUNK_FRAMES, None, copy=False) for b in range(B)], a.reps)
    elif which == "copy":
        dt = timed(lambda: [_format_device(atom14[b], aat, CHUNK_FRAMES, None) for b in range(B)], a.reps)
    else:
        with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
            dt = timed(lambda: [atom14_to_pdb(atom14[b], aat, os.path.join(td, f"{b}.pdb")) for b in range(B)], a.reps)
            size = sum(os.path.getsize(os.path.join(td, f)) for f in os.listdir(td))
            out.update(bytes=size, GB_per_s=size / dt / 1e9, directory=a.out_dir or tempfile.gettempdir())
    out.update(frames=B * M, seconds=dt, frames_per_s=B * M / dt, reps=a.reps)
    return out


def cli(a):
    """`sim_inference --synthetic --batch 16 --num_rollouts 10` (T 1000) on two groups, each timed in its two parts."""
    from mdgen_amd import pdb, sim_inference
    from mdgen_amd.geometry import restype_order, samples_to_atom14
    from mdgen_amd.rigid_utils import Rotation
    dev = torch.device("cuda")
    letters = "ARNDCQEGHILKMFPSTWYV"
    g = torch.Generator().manual_seed(3)
    names = ["".join(letters[int(i)] for i in torch.randint(0, 20, (4,), generator=g)) + f"{j}" for j in range(32)]
    groups = []   # two groups of 16: the first pays the graph capture, the second is the steady state
    inner_write, inner_sample = pdb.atom14_to_pdb, sim_inference.sample_group
    fmt = host_formatter(a.host_module)

    def sample(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner_sample(*args, **kw)
        torch.cuda.synchronize()
        groups.append({"sampling_s": time.perf_counter() - t0, "writing_s": 0.0})
        return out

    def writer(atom14, aatype, path):
        t0 = time.perf_counter()
        if a.writer == "host":   # what the drivers did before: the host copy, one Python string per atom
            with open(path, "w") as f:
                f.write(fmt(atom14.cpu().numpy(), np.asarray(aatype)))
        else:
            inner_write(atom14, aatype, path)
        groups[-1]["writing_s"] += time.perf_counter() - t0
    pdb.atom14_to_pdb, sim_inference.sample_group = writer, sample   # (run() looks both names up when it is called)
    with tempfile.TemporaryDirectory(dir=a.out_dir) as td:
        data = os.path.join(td, "data")
        os.makedirs(data)
        for n in names:
            q = torch.randn(1, 4, 4, generator=g)
            rot = Rotation(quats=(q / q.norm(dim=-1, keepdim=True)).to(dev)).get_rot_mats()
            tr = torch.cumsum(2.2 * torch.randn(1, 4, 3, generator=g), 1).to(dev)
            ang = 6.2831853 * torch.rand(1, 4, 7, generator=g)
            lat = torch.zeros(1, 1, 4, 21, device=dev)
            lat[..., 0] = 1.0
            lat[..., 7:21] = torch.stack([ang.sin(), ang.cos()], -1).reshape(1, 1, 4, 14).to(dev)
            a14 = samples_to_atom14(lat, rot, tr, torch.tensor([[restype_order[c] for c in n[:4]]], device=dev), tps=False)[0]
            np.save(os.path.join(data, f"{n}.npy"), a14.cpu().numpy().astype(np.float16))
        split = os.path.join(td, "split.csv")
        with open(split, "w") as f:
            f.write("name,seqres\n" + "".join(f"{n},{n[:4]}\n" for n in names))
        argv = ["--synthetic", "--data_dir", data, "--split", split, "--out_dir", os.path.join(td, "out"), "--batch", "16",
                "--num_rollouts", "10"]
        res = sim_inference.main(argv)
        size = sum(os.path.getsize(os.path.join(td, "out", f)) for f in os.listdir(os.path.join(td, "out")))
    for grp in groups:
        grp["wall_s"] = grp["sampling_s"] + grp["writing_s"]
    return {"leg": "cli", "writer": a.writer, "formatter": a.host_module or "this tree", "frames": res["frames"], "bytes": size,
            "first_group": groups[0], "second_group": groups[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES), default=None)
    ap.add_argument("--leg", choices=["host", "kernel", "copy", "file", "cli"], default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=1000, help="frames the host formatter is timed on")
    ap.add_argument("--host-module", default=None, help="a pdb.py whose frames_to_pdb_string the host legs time")
    ap.add_argument("--writer", choices=["device", "host"], default="device")
    ap.add_argument("--out-dir", default=None, help="where the file legs write (default: the system's temporary directory)")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if a.leg == "cli":
        print(json.dumps(cli(a)), flush=True)
        return
    for shape in ([a.shape] if a.shape else list(SHAPES)):
        for which in ([a.leg] if a.leg else ["host", "kernel", "copy", "file"]):
            print(json.dumps(leg(shape, which, a)), flush=True)


if __name__ == "__main__":
    main()
