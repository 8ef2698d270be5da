"""Multi-model PDB writer for sampled trajectories, byte-compatible with the reference's
`mdgen.utils.atom14_to_pdb` (utils.py:58-64 -> `create_full_prot` :67-92 -> `prots_to_pdb` :95-102 ->
`protein.to_pdb` protein.py:321-443), without mdtraj / Biopython.

Format (one block per frame):  `MODEL <i>` (0-based, unpadded), then one ATOM record per present atom in atom37
order (an atom is present when |x|+|y|+|z| > 1e-7, utils.py:77), a `TER` record, `ENDMDL`.  Records are padded
to 80 columns; residue numbers are 0-based, chain `A`, occupancy 1.00, B-factor 0.00, element = first letter of
the atom name (protein.py:388-413).

Two formatters write these bytes.  `frames_to_pdb_string` is the host one: a Python string per atom, a few thousand
frames a second -- the oracle of the other, and the path of NumPy arrays and CPU tensors.  `atom14_to_pdb` on a CUDA
tensor, which is what the three command-line drivers hand it, formats on the device (`mdgen_pdb_format`,
csrc/k_pdb.hip) from `record_templates` and appends the copied-back text to the file chunk by chunk: writing is on
the drivers' wall clock, and the array is on the device when the sampler returns.  The module imports without torch;
the device path imports torch and the library when it is taken."""
from __future__ import annotations

import os

import numpy as np

_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "residue_tables.npz")
_T = None

RECORD_BYTES = 81          # an 80-column record + "\n"
MAX_SERIAL = 99999         # five columns
MAX_RESIDUES = 9999        # mdgen_pdb_format's limit on L: four columns for the 0-based residue number (and a spare)
CHUNK_FRAMES = 4096        # frames per mdgen_pdb_format call of atom14_to_pdb's device path ...
CHUNK_BYTES = 1 << 28      # ... and the limit on its text buffer (one on the device, one pinned on the host)


def residue_tables():
    """Residue constant tables as numpy arrays (oracle/gen_residue_tables.py); no torch, no device library."""
    global _T
    if _T is None:
        d = np.load(_NPZ)
        _T = {k: d[k] for k in d.files}
    return _T


def atom14_to_atom37(atom14: np.ndarray, aatype: np.ndarray) -> np.ndarray:
    """geometry.py atom14_to_atom37: gather per residue type + mask.  atom14 [..., L, 14, 3], aatype [L]."""
    t = residue_tables()
    idx = np.asarray(t["atom37_to_atom14"])[aatype]                       # [L, 37]
    m = np.asarray(t["atom37_mask"])[aatype]                              # [L, 37]
    a37 = np.take_along_axis(atom14, np.broadcast_to(idx[..., None], atom14.shape[:-3] + idx.shape + (3,)), axis=-2)
    return a37 * m[..., None]


def _atom_record(serial, name, r3, i, xyz, element) -> str:
    """The ATOM record (protein.py:388-413), 80 columns: THE place its layout is written.  `serial`: an int, or "" for a
    template; `xyz`: the three %8.3f fields as one string (24 blanks for a template)."""
    return (f"{'ATOM':<6}{serial:>5} {name:<4}{'':>1}{r3:>3} {'A':>1}{i:>4}{'':>1}   "
            f"{xyz}{1.0:>6.2f}{0.0:>6.2f}          {element:>2}{'':>2}").ljust(80)


def _ter_record(serial, r3, i) -> str:
    """The TER record after a frame's last atom (protein.py:420-431), 80 columns; `serial` as in `_atom_record`."""
    return f"{'TER':<6}{serial:>5}      {r3:>3} {'A':>1}{i:>4}".ljust(80)


def _names():
    t = residue_tables()
    atom_types = [str(a) for a in t["atom_types"]]
    return atom_types, [a if len(a) == 4 else f" {a}" for a in atom_types], [str(r) for r in t["restype_3"]]


def _checked_aatype(aatype) -> np.ndarray:
    aatype = np.asarray(aatype).astype(np.int64)
    if aatype.ndim != 1 or aatype.shape[0] < 1:
        raise ValueError(f"aatype {aatype.shape}: expected [L]")
    if np.any(aatype > 20) or np.any(aatype < 0):
        raise ValueError("Invalid aatypes.")
    return aatype


def record_templates(aatype):
    """(uint8 [L, 37, 81], uint8 [81]): for every (residue i, atom37 slot k) the ATOM record + "\\n" with the serial
    (columns 7-11) and the coordinates (columns 31-54) blank, and the sequence's TER record + "\\n" with the serial blank --
    what `mdgen_pdb_format` copies and fills in.  Built with the format expressions `frames_to_pdb_string` uses.  Needs
    L <= 9999 + 1: beyond that the residue number widens the record."""
    aatype = _checked_aatype(aatype)
    atom_types, names, res3 = _names()
    L = aatype.shape[0]
    lines = [_atom_record("", names[k], res3[aatype[i]], i, " " * 24, atom_types[k][0]) + "\n"
             for i in range(L) for k in range(37)]
    ter = _ter_record("", res3[aatype[L - 1]], L - 1) + "\n"
    if any(len(s) != RECORD_BYTES for s in lines) or len(ter) != RECORD_BYTES:
        raise ValueError(f"L = {L}: a record is wider than 80 columns")
    tpl = np.frombuffer("".join(lines).encode("ascii"), dtype=np.uint8).reshape(L, 37, RECORD_BYTES).copy()
    return tpl, np.frombuffer(ter.encode("ascii"), dtype=np.uint8).copy()


def frames_to_pdb_string(atom14: np.ndarray, aatype: np.ndarray) -> str:
    """atom14 [M, L, 14, 3] (Angstrom), aatype [L] -> the text `atom14_to_pdb` writes."""
    atom_types, names, res3 = _names()
    atom14 = np.asarray(atom14, dtype=np.float32)
    aatype = np.asarray(aatype).astype(np.int64)
    if atom14.ndim != 4 or atom14.shape[-2:] != (14, 3) or atom14.shape[1] != aatype.shape[0]:
        raise ValueError(f"atom14 {atom14.shape} / aatype {aatype.shape}: expected [M,L,14,3] and [L]")
    if np.any(aatype > 20) or np.any(aatype < 0):
        raise ValueError("Invalid aatypes.")
    a37 = atom14_to_atom37(atom14, aatype)
    present = np.abs(a37).sum(-1) > 1e-7
    out = []
    L = aatype.shape[0]
    for m in range(a37.shape[0]):
        out.append(f"MODEL {m}")
        serial = 1
        for i in range(L):
            r3 = res3[aatype[i]]
            for k in range(37):
                if not present[m, i, k]:
                    continue
                x, y, z = a37[m, i, k]
                out.append(_atom_record(serial, names[k], r3, i, f"{x:>8.3f}{y:>8.3f}{z:>8.3f}", atom_types[k][0]))
                serial += 1
        out.append(_ter_record(serial, res3[aatype[L - 1]], L - 1))
        out.append("ENDMDL")
    return "\n".join(out) + "\n"


def pdb_to_atom14(path, aatype) -> np.ndarray:
    """The inverse of `atom14_to_pdb` for this project's own files: float32 [M, L, 14, 3] of the M models of `path`, the
    coordinates as printed (three decimals), absent atoms zero.  It reads the fixed columns `_atom_record` writes -- atom name
    13-16, residue number 23-26, x / y / z 31-54 -- and nothing else of the PDB format; host only, NumPy only."""
    t = residue_tables()
    aatype = _checked_aatype(aatype)
    L = aatype.shape[0]
    lines = open(path, "rb").read().split(b"\n")
    is_atom = np.fromiter((ln.startswith(b"ATOM") for ln in lines), bool, len(lines))
    is_model = np.fromiter((ln.startswith(b"MODEL") for ln in lines), bool, len(lines))
    M = int(is_model.sum())
    out = np.zeros((M, L, 14, 3), np.float32)
    if not is_atom.any():
        return out
    model = (np.cumsum(is_model) - 1)[is_atom]
    short = [i for i in np.nonzero(is_atom)[0] if len(lines[i]) < 54]
    if short or model.min() < 0:
        raise ValueError(f"{path}: an ATOM record is shorter than 54 columns, or stands in front of the first MODEL line")
    rec = np.frombuffer(b"".join(lines[i][:54] for i in np.nonzero(is_atom)[0]), np.uint8).reshape(-1, 54)
    res = np.ascontiguousarray(rec[:, 22:26]).view("S4").ravel().astype(np.int64)
    names = np.char.strip(np.ascontiguousarray(rec[:, 12:16]).view("S4").ravel())
    k37_of = {str(a).encode(): k for k, a in enumerate(t["atom_types"])}
    uniq, inv = np.unique(names, return_inverse=True)
    unknown = [u.decode() for u in uniq if u not in k37_of]
    if unknown or res.min() < 0 or res.max() >= L:
        raise ValueError(f"{path}: atom names {unknown} or residue numbers outside 0 .. {L - 1}: not this sequence's file")
    k37 = np.array([k37_of[u] for u in uniq], np.int64)[inv]
    aa = aatype[res]
    if not np.all(np.asarray(t["atom37_mask"])[aa, k37] > 0):
        raise ValueError(f"{path}: an atom that its residue type does not have: not this sequence's file")
    slot = np.asarray(t["atom37_to_atom14"])[aa, k37]
    for c in range(3):
        out[model, res, slot, c] = np.ascontiguousarray(rec[:, 30 + 8 * c:38 + 8 * c]).view("S8").ravel().astype(np.float64)
    return out


def sequence_atoms(aatype) -> int:
    """Atoms `atom37_mask` gives the sequence: the most ATOM records a frame can have."""
    return int(np.asarray(residue_tables()["atom37_mask"])[_checked_aatype(aatype)].sum())


def frame_capacity(aatype) -> int:
    """Upper bound on one frame's bytes: the longest MODEL line (27), a record per atom of the sequence and the TER
    record, ENDMDL (7) -- how `mdgen_pdb_format`'s caller sizes `text`."""
    return 27 + RECORD_BYTES * (sequence_atoms(aatype) + 1) + 7


def sequence_inputs(aatype: np.ndarray, device):
    """The sequence's inputs of `mdgen_pdb_format` on `device`: aatype, the two residue tables, the templates."""
    import torch
    from .geometry import residue_tables as device_tables
    tb = device_tables(device)
    tpl, ter = record_templates(aatype)
    return (torch.from_numpy(aatype).to(device), tb["atom37_to_atom14"], tb["atom37_mask"],
            torch.from_numpy(tpl).to(device), torch.from_numpy(ter).to(device))


def format_frames_device(atom14, seq_inputs, model_base, offsets, text, status) -> None:
    """One `mdgen_pdb_format` call on `atom14`'s device and current stream: atom14 (M, L, 14, 3) fp32 contiguous, `seq_inputs`
    from `sequence_inputs`; offsets int64 [>= M + 1], text uint8, status int64 [2] are written (include/mdgen_amd.h)."""
    import torch
    from ._lib import launch, lib, ptr
    aat, a37to14, a37mask, tpl, ter = seq_inputs
    M, L = int(atom14.shape[0]), int(atom14.shape[1])
    if offsets.numel() < M + 1 or status.numel() < 2:
        raise ValueError("offsets needs M + 1 elements, status 2")
    launch(lib.mdgen_pdb_format, atom14, M, L, int(model_base), ptr(atom14, torch.float32), ptr(aat, torch.int64),
           ptr(a37to14, torch.int64), ptr(a37mask, torch.float32), ptr(tpl, torch.uint8), ptr(ter, torch.uint8),
           ptr(offsets, torch.int64), ptr(text, torch.uint8), int(text.numel()), ptr(status, torch.int64))


def _format_device(atom14, aatype: np.ndarray, chunk: int, sink, copy: bool = True) -> bool:
    """`atom14_to_pdb`'s device path: the text of atom14 (M, L, 14, 3; fp32, contiguous, on the GPU), chunk by chunk, into the
    binary file object `sink`.  False when a field of the trajectory overflows: what `sink` holds by then is to be discarded.
    `sink` None: nothing is written, and with `copy` False nothing is copied back either (scripts/pdb_bench.py times the parts)."""
    import torch
    M = int(atom14.shape[0])
    per_frame = frame_capacity(aatype)
    chunk = max(1, min(int(chunk), M, CHUNK_BYTES // per_frame))
    seq = sequence_inputs(aatype, atom14.device)
    text = torch.empty(chunk * per_frame, dtype=torch.uint8, device=atom14.device)
    offsets = torch.empty(chunk + 1, dtype=torch.int64, device=atom14.device)
    status = torch.empty(2, dtype=torch.int64, device=atom14.device)
    host = torch.empty(chunk * per_frame if copy else 0, dtype=torch.uint8, pin_memory=True)
    host_np = host.numpy()
    for m0 in range(0, M, chunk):
        format_frames_device(atom14[m0:m0 + chunk], seq, m0, offsets, text, status)
        bad, total = (int(v) for v in status.cpu())   # (the one read-back; it waits for the three kernels)
        if bad > 0:
            return False
        assert 0 < total <= text.numel(), (total, text.numel())
        if copy:
            host[:total].copy_(text[:total], non_blocking=True)
            torch.cuda.current_stream(atom14.device).synchronize()
            if sink is not None:
                sink.write(memoryview(host_np[:total]))
    return True


def atom14_to_pdb(atom14, aatype, path, chunk: int = CHUNK_FRAMES) -> None:
    """Drop-in for `mdgen.utils.atom14_to_pdb(atom14, aatype, path)`: atom14 [M, L, 14, 3] (Angstrom), aatype [L].

    A CUDA tensor is formatted on its device, `chunk` frames per call (and at most CHUNK_BYTES of text), each chunk copied
    to pinned memory and appended to the file.  A trajectory with a field that overflows its columns (a coordinate outside
    %8.3f's eight, more than 99 999 atoms or 9 999 residues a frame) is written by the host formatter instead, whole, so that
    such fields come out as they always did.  A NumPy array or a CPU tensor takes the host formatter."""
    if getattr(atom14, "is_cuda", False):
        import torch
        aat = aatype.cpu().numpy() if hasattr(aatype, "cpu") else aatype
        aat = _checked_aatype(aat)
        if atom14.ndim != 4 or tuple(atom14.shape[-2:]) != (14, 3) or atom14.shape[1] != aat.shape[0]:
            raise ValueError(f"atom14 {tuple(atom14.shape)} / aatype {aat.shape}: expected [M,L,14,3] and [L]")
        if atom14.shape[0] == 0:
            atom14 = atom14.cpu()
        else:
            dev = atom14.to(torch.float32).contiguous()
            fits = aat.shape[0] <= MAX_RESIDUES and sequence_atoms(aat) + 1 <= MAX_SERIAL   # (+ 1: the TER record's serial)
            if fits:
                with open(path, "wb") as f:
                    if _format_device(dev, aat, chunk, f):
                        return
            atom14 = dev.cpu()
        aatype = aat
    with open(path, "w") as f:
        f.write(frames_to_pdb_string(np.asarray(atom14), np.asarray(aatype)))
