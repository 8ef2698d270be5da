"""mdgen_pdb_format without a device: the entry point's binding and refusals, and its algorithm -- tests/pdb_ref.py, a NumPy
restatement of the count, scan and format passes over mdgen_amd.pdb.record_templates -- against frames_to_pdb_string byte for
byte, on the reference's golden trajectory and on the edge arrays tests/test_pdb_gpu.py runs through the kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pdb_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_header_exports_and_binding_agree():
    import mdgen_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    decl = re.search(r"int32_t mdgen_pdb_format\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    params = [p.strip() for p in decl.split(",")]
    kinds = [ctypes.c_void_p if "*" in p else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[p.split()[0]] for p in params]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "M", "L", "model_base", "atom14", "aatype", "atom37_to_atom14", "atom37_mask", "templates", "ter_template", "offsets",
        "text", "text_capacity", "status", "stream"]
    assert "mdgen_pdb_format" in L.EXPORTS
    assert list(L.lib.mdgen_pdb_format.argtypes) == kinds and L.lib.mdgen_pdb_format.restype is ctypes.c_int32
    assert L.lib.mdgen_abi_version() == L.ABI_VERSION == 8   # an addition: no signature or struct changed


def test_refusals_without_a_device():
    import mdgen_amd._lib as L
    f = L.lib.mdgen_pdb_format
    buf = (ctypes.c_uint8 * 64)()   # never dereferenced: every refusal is decided on the host before a device call
    p = ctypes.addressof(buf)
    ok = [p] * 8
    for hole in range(8):
        assert f(1, 1, 0, *[None if j == hole else p for j in range(8)], 64, p, None) == -1, hole
        assert b"null" in L.lib.mdgen_last_error()
    assert f(1, 1, 0, *ok, 64, None, None) == -1
    for M, L_, base in ((0, 1, 0), (-1, 1, 0), (1, 0, 0), (1, 10000, 0), (1, 1, -1), (2, 1, 2 ** 63 - 1)):
        assert f(M, L_, base, *ok, 64, p, None) == -2, (M, L_, base)
    assert f(1, 1, 0, *ok, -1, p, None) == -2


def test_record_templates():
    from mdgen_amd.pdb import frame_capacity, record_templates, sequence_atoms
    aatype = np.array([R.SER, R.TRP, 20])
    tpl, ter = record_templates(aatype)
    assert tpl.shape == (3, 37, 81) and tpl.dtype == np.uint8 and ter.shape == (81,) and ter.dtype == np.uint8
    rec = tpl[1, 1].tobytes().decode()   # TRP, atom37 slot 1 = CA
    assert rec == "ATOM         CA  TRP A   1    " + " " * 24 + "  1.00  0.00           C  \n"
    assert ter.tobytes().decode() == ("TER   " + " " * 5 + " " * 6 + "UNK A   2").ljust(80) + "\n"
    assert (tpl[..., 80] == 10).all() and (tpl[..., 6:11] == 32).all() and (tpl[..., 30:54] == 32).all()
    assert sequence_atoms(aatype) == 6 + 14 and frame_capacity(aatype) == 27 + 81 * 21 + 7
    with pytest.raises(ValueError):
        record_templates(np.array([21]))
    with pytest.raises(ValueError):
        record_templates(np.zeros(10001, np.int64))   # residue number 10000: five columns


def _check(atom14, aatype, model_base=0):
    want, want_off = R.host_text(atom14, aatype, model_base)
    got, off, bad = R.device_text(atom14, aatype, model_base)
    assert bad == 0
    assert np.array_equal(off, want_off)
    assert got == want
    return got


def test_restatement_reproduces_the_golden_trajectory():
    g = np.load(os.path.join(GOLDEN, "pdb_small.npz"))
    assert _check(g["atom14"], g["aatype"]) == bytes(g["text"])   # the reference's own bytes


def test_restatement_rounding():
    a, aatype = R.rounding_case()
    pres, _ = R.presence(a, aatype)
    assert pres[:, 0, [0, 1, 2, 3, 4]].all()   # N, CA, C, CB, O of ALA: every value of the list is printed
    text = _check(a, aatype).decode()
    assert "   0.062" in text and "   0.188" in text and "  -0.062" in text and "  -0.000" in text and "   0.002" in text
    assert " 999.999" in text and "-999.999" in text and "9999.998" in text
    assert "   0.000   1.000   1.000" in text   # (1e-30, 1, 1)
    assert R.coord_field(-1e-4) == b"  -0.000" and R.coord_field(-0.0) == b"  -0.000" and R.coord_field(0.0015) == b"   0.002"


def test_restatement_presence_boundary_has_both_outcomes():
    from mdgen_amd.pdb import atom14_to_atom37, residue_tables
    a, aatype = R.presence_case()
    _check(a, aatype)
    pres, _ = R.presence(a, aatype)
    host = np.abs(atom14_to_atom37(a, aatype)).sum(-1) > 1e-7   # the host writer's own expression
    assert np.array_equal(pres, host)
    idx, mask = residue_tables()["atom37_to_atom14"][R.TRP], residue_tables()["atom37_mask"][R.TRP]
    # the atom37 slot of TRP's atom14 slot 2 + j, which holds triple j in frame 4
    outcomes = [bool(host[4, 1, [k for k in range(37) if mask[k] and idx[k] == 2 + j][0]]) for j in range(len(R.PRESENCE_TRIPLES))]
    assert True in outcomes and False in outcomes, outcomes
    assert outcomes[0] is False and outcomes[2] is True and outcomes[3] is True   # 1e-7 is not > 1e-7; 1.1e-7 and 1.2e-7 are
    sizes = np.diff(R.host_text(a, aatype)[1])
    assert len(set(sizes.tolist())) >= 4 and sizes[5] == len("MODEL 5\n") + 81 + 7


def test_restatement_residue_types_model_digits_and_launch_edges():
    for a, aatype in R.types_cases():
        _check(a, aatype)
    gly = np.array([R.GLY])
    _check(R.plausible(1001, 1, seed=5), gly)
    _check(R.plausible(4, 1, seed=6), gly, model_base=9998)
    for L_ in (1, 2, 7, 19, 33, 64, 65):   # (L = 256 runs on the GPU only: the same code path, 9 000 Python records a frame)
        _check(*R.launch_edge_case(3, L_))


@pytest.mark.parametrize("name", list(R.REFUSED))
def test_restatement_refuses_what_has_no_field(name):
    a, aatype = R.refusal_case(name)
    text, _, bad = R.device_text(a, aatype)
    assert bad >= 1 and text == b""
    assert not R.fits(np.float32(R.REFUSED[name]))
    assert R.fits(np.float32(-999.9994)) and R.fits(np.float32(9999.998)) and R.rounded(np.float32(-999.9995)) == -1000000


def test_atom14_to_pdb_host_path_is_unchanged(tmp_path):
    import torch
    from mdgen_amd.pdb import atom14_to_pdb, frames_to_pdb_string
    g = np.load(os.path.join(GOLDEN, "pdb_small.npz"))
    want = frames_to_pdb_string(g["atom14"], g["aatype"])
    for tag, arr, aat in (("numpy", g["atom14"], g["aatype"]), ("tensor", torch.from_numpy(g["atom14"]), torch.from_numpy(g["aatype"]))):
        p = tmp_path / f"{tag}.pdb"
        atom14_to_pdb(arr, aat, p)
        assert open(p).read() == want, tag
