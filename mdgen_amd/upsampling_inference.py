"""Trajectory-upsampling driver, command-line compatible with the reference's `upsampling_inference.py:1-10`
(`--ckpt --data_dir --suffix --pdb_id --batch_size --out_dir --split`), plus

  --num_steps S      Euler steps per window (a non-Euler checkpoint is refused unless S or --sampling_method is given);
  --sampling_method {euler,dopri5,midpoint,heun3,rk4,sde,sde_heun}   the solver: dopri5 is the reference's adaptive default (torchdiffeq,
                     atol 1e-6, rtol 1e-3; one step size per call, shared by a --batch_size group); euler without --num_steps
                     takes the reference's 49-step grid; midpoint / heun3 / rk4: torchdiffeq's fixed-grid solvers with
                     --num_steps steps (default 24 / 16 / 12 = 48 network evaluations);
  --precision {bf16,fp32}, --npy (also save the sampled array), --xtc (as `sim_inference.py`: refused before sampling
                     where mdtraj is missing);
  --synthetic        seeded weights instead of --ckpt, with --num_frames T / --cond_interval c (a checkpoint supplies both);
  --superpose        the written trajectory (PDB and --npy) is superposed on its own first frame over its existing atoms, on the
                     device before it is formatted (`mdgen_ens_superpose`; the reference's `traj.superpose(traj)`).  Off by default.

Under `torch.distributed.run` the names of the split are sharded over the ranks (`sim_inference.dist_env` / `select_names`).

Per name: `{data_dir}/{name}{suffix}.npy` holds KEY FRAMES only, [N_key, L, 14, 3], one every `cond_interval` frames of the
trajectory.  Frames and torsions of all key frames are computed on the device (`mdgen_atom14_to_cond`, key frames as the batch
axis), cut into windows of K = T / c key frames (`split_windows`; a trailing partial window is dropped, as
upsampling_inference.py:47-66 does), and the windows are sampled `batch_size` at a time through
`NewMDGenWrapper.upsample` -- windows are the batch axis of one library call, the key frames never expand into a (B, T, L)
window of zeros.  Output: `{out_dir}/{name}.pdb` with all n_windows * T frames in order.  Within a window the last c - 1 frames
have no right-hand key frame (the next window's first key frame is not part of it): the reference's behaviour, kept.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from .solver import add_solver_arguments, solver_kwargs


def split_windows(n_key: int, num_frames: int, cond_interval: int):
    """(n_windows, K): `n_key` key frames, one every `cond_interval` frames, cut into windows of `num_frames` frames.
    K = num_frames // cond_interval key frames per window, window i takes key frames [i*K, (i+1)*K); the key frames left
    over after the last whole window are dropped (upsampling_inference.py:47-66).  `num_frames` must be a multiple of
    `cond_interval`: otherwise a window's [::cond_interval] rows outnumber its K key frames (the reference's slice
    assignment fails there too)."""
    n_key, T, c = int(n_key), int(num_frames), int(cond_interval)
    if n_key < 0 or T < 1 or c < 1:
        raise ValueError(f"n_key >= 0, num_frames >= 1 and cond_interval >= 1 are required, got {n_key}, {T}, {c}")
    if T % c != 0:
        raise ValueError(f"num_frames={T} is not a multiple of cond_interval={c}: a window's key frames would not line up "
                         "with the next window's")
    return (n_key * c) // T, T // c


def key_frame_windows(arr, seqres_str, num_frames, cond_interval, device):
    """Key-frame atom14 [N_key, L, 14, 3] -> the key-frame batch of all whole windows: torsions (W,K,L,7,2), trans
    (W,K,L,3), rots (W,K,L,3,3), seqres (W,L), mask (W,L) with W = n_windows."""
    from .geometry import atom14_to_cond, restype_order
    n_windows, K = split_windows(arr.shape[0], num_frames, cond_interval)
    used = n_windows * K
    seq = torch.tensor([restype_order[ch] for ch in seqres_str], device=device)
    L_ = seq.shape[0]
    if used == 0:
        return None
    a = torch.from_numpy(np.copy(arr[:used]).astype(np.float32)).to(device)
    c = atom14_to_cond(a, seq[None].expand(used, L_))
    return {"torsions": c["torsions"].view(n_windows, K, L_, 7, 2), "trans": c["trans"].view(n_windows, K, L_, 3),
            "rots": c["rots"].view(n_windows, K, L_, 3, 3), "seqres": seq[None].expand(n_windows, L_).contiguous(),
            "mask": torch.ones(n_windows, L_, device=device)}


def upsample_name(model, windows, args, name_index=0):
    """All windows of one name, `batch_size` at a time -> atom14 (n_windows * T, L, 14, 3).  `name_index`: the name's index within
    the split; with --sde_seed window i draws its generated noise at (sample i, block name_index), whichever rank and batch size
    sample it."""
    W = windows["trans"].shape[0]
    kw = solver_kwargs(args)
    out = []
    for i in range(0, W, max(1, args.batch_size)):
        kb = {k: v[i:i + args.batch_size] for k, v in windows.items()}
        if "rng_seed" in kw:
            kw.update(rng_sample_base=i, rng_block_base=name_index)
        atom14, _ = model.upsample(kb, **kw)
        if kw.get("sampling_method") == "dopri5":
            st = model.last_stats
            print(f"dopri5: {st['nfe']} network evaluations ({st['accepted']} accepted, {st['rejected']} rejected steps)")
        out.append(atom14.reshape(-1, *atom14.shape[2:]))
    return torch.cat(out, 0)


def run(args, model, device, names_seqres, rank=0, world=1, sync=None):
    """The driver proper (upsampling_inference.py:68-102), given a loaded model: this process's names (rank shard,
    --pdb_id) -> `{out_dir}/{name}.pdb`.  `names_seqres`: ordered {name: sequence} of the whole split."""
    from .geometry import restype_order
    from .pdb import atom14_to_pdb
    from .sim_inference import require_xtc_writer, select_names, write_xtc
    sync = sync or (lambda: None)
    if getattr(args, "xtc", False):
        require_xtc_writer()
    T, c = int(model.args.num_frames), int(model.args.cond_interval)
    split_windows(0, T, c)   # refuse T % c != 0 before anything is read
    names = select_names(list(names_seqres), args.pdb_id, 0, 1, rank, world)
    os.makedirs(args.out_dir, exist_ok=True)
    done, total_frames, total_s = [], 0, 0.0
    split_index = {n: i for i, n in enumerate(names_seqres)}
    for name in names:
        arr = np.lib.format.open_memmap(f"{args.data_dir}/{name}{args.suffix}.npy", "r")
        windows = key_frame_windows(arr, names_seqres[name], T, c, device)
        if windows is None:
            print(f"{name}: {arr.shape[0]} key frames are fewer than one window of {T // c}; nothing to sample")
            continue
        sync()
        start = time.time()
        atom14 = upsample_name(model, windows, args, **({} if getattr(args, "sde_seed", None) is None
                                                        else {"name_index": split_index[name]}))
        sync()
        dur = time.time() - start
        nfr = atom14.shape[0]
        total_frames, total_s = total_frames + nfr, total_s + dur
        print(f"{name}: {nfr / dur:.1f} frames/s ({dur:.3f} s, {windows['trans'].shape[0]} windows of {T} frames, "
              f"batch {args.batch_size})")
        aat = np.array([restype_order[ch] for ch in names_seqres[name]])
        if getattr(args, "superpose", False):
            from .ensemble import superpose_on_first
            atom14 = superpose_on_first(atom14, aat)
        # a device tensor is formatted on the device (pdb.py); the host copy is made only for what needs one
        host = atom14.cpu().numpy() if args.npy or not atom14.is_cuda else None
        path = os.path.join(args.out_dir, f"{name}.pdb")
        atom14_to_pdb(atom14 if atom14.is_cuda else host, aat, path)
        if getattr(args, "xtc", False):
            write_xtc(path, os.path.join(args.out_dir, f"{name}.xtc"))
        if args.npy:
            np.save(os.path.join(args.out_dir, f"{name}.npy"), host)
        done.append(name)
    return {"names": done, "frames": total_frames, "seconds": total_s}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt", type=str, default=None)
    p.add_argument("--data_dir", type=str, default=None, required=True)
    p.add_argument("--suffix", type=str, default="_i100")
    p.add_argument("--pdb_id", nargs="*", default=[])
    p.add_argument("--batch_size", type=int, default=1, help="windows per upsample() call")
    p.add_argument("--out_dir", type=str, default=".")
    p.add_argument("--split", type=str, default="splits/4AA_implicit_test.csv")
    add_solver_arguments(p, per="window")
    p.add_argument("--precision", choices=["bf16", "fp32"], default="bf16",
                   help="bf16 MFMA operands (default) or the fp32-operand tolerance mode (~10x slower)")
    p.add_argument("--xtc", action="store_true")
    p.add_argument("--npy", action="store_true", help="also save the sampled atom14 array as .npy")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic weights instead of --ckpt")
    p.add_argument("--num_frames", type=int, default=None, help="frames per window (only with --synthetic; default 1000)")
    p.add_argument("--cond_interval", type=int, default=None,
                   help="frames between key frames (only with --synthetic; default 100)")
    p.add_argument("--superpose", action="store_true", help="superpose each written trajectory (PDB and --npy) on its own first frame over its existing atoms, on the device "
                        "(the reference's traj.superpose(traj))")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    solver_kwargs(args, p.error)
    if not args.synthetic and (args.num_frames is not None or args.cond_interval is not None):
        p.error("--num_frames / --cond_interval go with --synthetic only (a checkpoint supplies its own)")
    if not args.synthetic and not args.ckpt:
        p.error("--ckpt is required (or --synthetic)")
    if args.batch_size < 1:
        p.error("--batch_size must be >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    import pandas as pd
    from .config import ModelConfig
    from .sim_inference import dist_env
    from .synthetic import synth_state_dict
    from .wrapper import NewMDGenWrapper, default_args
    rank, world, local_rank = dist_env()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    if args.synthetic:
        T = 1000 if args.num_frames is None else args.num_frames
        cfg = ModelConfig.forward_sim(num_frames=T)
        margs = default_args(cfg)
        margs.cond_interval = 100 if args.cond_interval is None else args.cond_interval
        if margs.cond_interval < 1 or T < 1:
            raise SystemExit("--num_frames and --cond_interval must be >= 1")
        model = NewMDGenWrapper(margs, device=device, precision=args.precision)
        model.model.load_state_dict(synth_state_dict(cfg, 0))
    else:
        model = NewMDGenWrapper.load_from_checkpoint(args.ckpt, device=device, precision=args.precision)
        if not getattr(model.args, "cond_interval", None):
            raise SystemExit("--ckpt is not an upsampling model (trained without --cond_interval)")
    try:
        split_windows(0, model.args.num_frames, model.args.cond_interval)
    except ValueError as e:
        raise SystemExit(str(e))
    df = pd.read_csv(args.split, index_col="name")
    names_seqres = {str(n): df.seqres[n] for n in df.index}
    return run(args, model, device, names_seqres, rank, world, sync=torch.cuda.synchronize)


if __name__ == "__main__":
    with torch.no_grad():
        main()
