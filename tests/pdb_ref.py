"""The two passes of mdgen_pdb_format (csrc/k_pdb.hip) restated in NumPy, and the edge arrays its tests share.

`device_text` computes, with integer arithmetic only, what the kernels compute: presence in fp32 in the kernel's order,
frame sizes and int64 offsets, the rounding rule n = rint((double) x * 1000) and the fill of the host-built record templates
(mdgen_amd.pdb.record_templates).  tests/test_pdb_device_cpu.py holds it against frames_to_pdb_string byte for byte -- the
algorithm without the HIP code -- and tests/test_pdb_gpu.py holds the kernels against the same oracle on the same arrays."""
import numpy as np

from mdgen_amd.pdb import RECORD_BYTES, atom14_to_atom37, frames_to_pdb_string, record_templates

ALA, GLY, SER, TRP = 0, 7, 15, 17   # residue_constants.restypes order ARNDCQEGHILKMFPSTWYV


# ---- the algorithm --------------------------------------------------------------------------------------------------
def presence(atom14, aatype):
    """bool [M, L, 37] and the masked atom37 positions: (|x| + |y|) + |z| > 1e-7f, every operation in fp32."""
    a37 = atom14_to_atom37(np.asarray(atom14, np.float32), np.asarray(aatype, np.int64)).astype(np.float32)
    ab = np.abs(a37)
    s = (ab[..., 0] + ab[..., 1]).astype(np.float32) + ab[..., 2]
    assert s.dtype == np.float32
    return s > np.float32(1e-7), a37


def rounded(x):
    """n = rint((double) x * 1000): ties to even on an exact product."""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * 1000.0)


def fits(x):
    """A coordinate has an %8.3f field of eight columns."""
    n = rounded(x)
    with np.errstate(invalid="ignore"):
        return np.isfinite(np.asarray(x, np.float32)) & (n >= -999999) & (n <= 9999999)


def coord_field(x) -> bytes:
    """The kernel's digits for one coordinate that fits."""
    x = np.float32(x)
    a = int(abs(rounded(x)))
    s = ("-" if np.signbit(x) else "") + str(a // 1000) + "." + "%03d" % (a % 1000)
    assert len(s) <= 8
    return s.rjust(8).encode()


def device_text(atom14, aatype, model_base=0):
    """(text bytes, offsets int64 [M + 1], bad): what the count, scan and format passes produce."""
    atom14 = np.asarray(atom14, np.float32)
    aatype = np.asarray(aatype, np.int64)
    M, L = atom14.shape[:2]
    tpl, ter = record_templates(aatype)
    pres, a37 = presence(atom14, aatype)
    n = pres.reshape(M, -1).sum(1)
    bad = int((~fits(a37)).sum()) + int((n + 1 > 99999).sum())
    sizes = np.array([len("MODEL %d\n" % (model_base + m)) for m in range(M)], np.int64) + RECORD_BYTES * (n + 1) + len("ENDMDL\n")
    offsets = np.zeros(M + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    if bad:
        return b"", offsets, bad
    out = bytearray()
    for m in range(M):
        out += b"MODEL %d\n" % (model_base + m)
        serial = 0
        for i, k in zip(*np.nonzero(pres[m])):
            rec = bytearray(tpl[i, k].tobytes())
            serial += 1
            rec[6:11] = b"%5d" % serial
            for c in range(3):
                rec[30 + 8 * c:38 + 8 * c] = coord_field(a37[m, i, k, c])
            out += rec
        rec = bytearray(ter.tobytes())
        rec[6:11] = b"%5d" % (serial + 1)
        out += rec + b"ENDMDL\n"
        assert len(out) == offsets[m + 1]
    return bytes(out), offsets, 0


# ---- the oracle -----------------------------------------------------------------------------------------------------
def host_text(atom14, aatype, model_base=0):
    """(bytes, offsets) of frames model_base .. model_base + M - 1 as frames_to_pdb_string writes them: the frames are put
    behind `model_base` empty ones (no atoms: three lines each), and the text of those is cut off."""
    atom14 = np.asarray(atom14, np.float32)
    full = np.concatenate([np.zeros((model_base,) + atom14.shape[1:], np.float32), atom14]) if model_base else atom14
    frames = frames_to_pdb_string(full, aatype).encode().split(b"ENDMDL\n")[model_base:-1]
    lens = np.array([len(f) + 7 for f in frames], np.int64)
    return b"ENDMDL\n".join(frames) + b"ENDMDL\n", np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- edge arrays ----------------------------------------------------------------------------------------------------
def mixed_types(L):
    return (np.arange(L) * 7 + 3) % 20


def plausible(M, L, seed=0):
    """Coordinates of the size a peptide has, every atom14 slot filled."""
    return (np.random.default_rng(seed).normal(size=(M, L, 14, 3)) * 12.0).astype(np.float32)


ROUNDING_VALUES = ([(2 * k + 1) / 16 for k in range(-200, 201)]            # exact ties, among them 0.0625 -> 0.062, 0.1875 -> 0.188
                   + [0.0, -0.0, 1e-4, -1e-4, -4.9e-4, 5e-4, -5e-4, 0.0015, 999.9994, -999.9994, 9999.998])


def rounding_case():
    """L = 1, ALA (five atoms): the values above cycle through the fifteen coordinates of a frame; the last frame's last atom
    is (1e-30, 1, 1)."""
    vals = np.array(ROUNDING_VALUES, np.float32)
    M = -(-(len(vals) + 3) // 15)
    a = np.zeros((M, 1, 14, 3), np.float32)
    a[:, 0, :5] = np.resize(vals, (M, 5, 3))
    a[-1, 0, 4] = (1e-30, 1.0, 1.0)
    return a, np.array([ALA])


PRESENCE_TRIPLES = [(1e-7, 0, 0), (4e-8, 3e-8, 3e-8), (4e-8, 4e-8, 3e-8), (-6e-8, 6e-8, 0)]


def presence_case():
    """L = 3 (SER, TRP, GLY), M = 6: atoms at exactly (0, 0, 0) in some frames only (frame sizes differ, serials shift), and the
    boundary triples of the presence test in frame 4."""
    a = plausible(6, 3, seed=1)
    a[1, 0, 2] = 0
    a[1, 1, 0] = 0
    a[3, 1, 5:9] = 0
    a[3, 2, 3] = 0
    a[5] = 0                                  # a frame without atoms
    for j, t in enumerate(PRESENCE_TRIPLES):
        a[4, 1, 2 + j] = t
    return a, np.array([SER, TRP, GLY])


def types_cases():
    """L = 21, every residue type once: type 20 (no atoms) last, where it supplies the TER record; and an order ending in TRP."""
    order = np.arange(21)
    return [(plausible(2, 21, seed=2), order), (plausible(2, 21, seed=3), np.array([*range(17), 18, 19, 20, TRP]))]


def launch_edge_case(M, L):
    """Records per frame on both sides of 64 and 256 (a wave walks a frame's slots 64 at a time); L = 7 is all TRP: 98 records."""
    aatype = np.full(7, TRP) if L == 7 else mixed_types(L)
    return plausible(M, L, seed=100 + L), aatype


REFUSED = {"10000.0": 10000.0, "-999.9995": -999.9995, "nan": float("nan"), "inf": float("inf")}


def refusal_case(name):
    """One coordinate without a field, at one atom of one frame."""
    a = plausible(3, 2, seed=4)
    a[1, 1, 1, 2] = REFUSED[name]
    return a, np.array([GLY, SER])
