"""The SE(3), pre/post-processing and loss kernels alone (csrc/k_se3.hip: k_rigid_compose, k_rigid_invert, k_rigid_apply,
k_quat_to_rot, k_rot_to_quat, k_from_3_points, k_prep_latents, k_samples_to_atom14, k_atom14_to_cond; csrc/k_small.hip: k_path_plan,
k_masked_mse; k_rel7's arithmetic through prep_latents(tps = 1) and rot_to_quat) through their `mdgen_*` entries, against the oracle's
own functions in fp64 on the device's fp32 inputs, at the cases of se3_ref.CASES: the 256-thread launch edge of every kernel, frame
boundaries inside a block, rotations at and near pi and the identity, every quaternion component dominant, T = 1, every
cond_interval against T, unnormalised quaternions and torsion pairs, per-sample start frames, every residue type, 100 A coordinates,
the unrolled loop's boundaries of the masked loss.  Every output starts as NaN (the int64 mask as -1) with 64 guard elements of 0xFF
bytes behind it.  The gate of every quantity is 32 x the error of torch's own fp32 against the same fp64 reference
(se3_ref.reference); tests/test_se3_kernels_cpu.py shows what the gates and the exact assertions catch."""
import ctypes as C

import pytest
import torch

import se3_ref as SR

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch.device("cuda")


class _Outputs:
    """Device outputs of one case: NaN (int64: -1) filled, each followed by SR.GUARD elements of 0xFF bytes."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def new(self, name, *shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        buf = torch.empty(n + SR.GUARD, dtype=dtype, device=self.dev)
        buf.view(torch.uint8).fill_(255)
        buf[:n] = -1 if dtype == torch.int64 else float("nan")
        self.bufs[name] = (buf, n, shape)
        return buf

    def collect(self):
        """Synchronise, check every guard, -> {name: CPU tensor}."""
        torch.cuda.synchronize()
        out = {}
        for name, (buf, n, shape) in self.bufs.items():
            assert bool((buf[n:].view(torch.uint8) == 255).all()), f"a kernel wrote behind {name}"
            out[name] = buf[:n].view(*shape).cpu()
        return out


def _algebra(L, c, g, o):
    n, lib, p, s = c.n, L.lib, L.ptr, L.stream_ptr()
    L.check(lib.mdgen_rigid_compose(n, p(g["R1"]), p(g["t1"]), p(g["R2"]), p(g["t2"]), p(o.new("comp_R", n, 3, 3)), p(o.new("comp_t", n, 3)), s))
    iR, it = o.new("inv_R", n, 3, 3), o.new("inv_t", n, 3)
    L.check(lib.mdgen_rigid_invert(n, p(g["R1"]), p(g["t1"]), p(iR), p(it), s))
    for name, inverse in (("apply", 0), ("inv_apply", 1)):
        L.check(lib.mdgen_rigid_apply(n, 1, p(g["R1"]), p(g["t1"]), p(g["p"]), p(o.new(name, n, 3)), inverse, s))
    L.check(lib.mdgen_quat_to_rot(n, p(g["q"]), 0, p(o.new("q2r_raw", n, 3, 3)), s))
    L.check(lib.mdgen_quat_to_rot(n, p(g["q"]), 1, p(o.new("q2r_norm", n, 3, 3)), s))
    L.check(lib.mdgen_from_3_points(n, p(g["p3a"]), p(g["p3b"]), p(g["p3c"]), p(o.new("f3_R", n, 3, 3)), p(o.new("f3_t", n, 3)), s))
    L.check(lib.mdgen_rot_to_quat(n, p(g["R1"]), p(o.new("quat", n, 4)), s))
    # A o A^-1 with the device's own inverse (the guards keep iR / it contiguous views of n frames)
    L.check(lib.mdgen_rigid_compose(n, p(g["R1"]), p(g["t1"]), p(iR), p(it), p(o.new("ident_R", n, 3, 3)), p(o.new("ident_t", n, 3)), s))


def _apply(L, c, g, o):
    for name, inverse in (("apply", 0), ("inv_apply", 1)):
        L.check(L.lib.mdgen_rigid_apply(c.n, c.ppf, L.ptr(g["R"]), L.ptr(g["t"]), L.ptr(g["p"]), L.ptr(o.new(name, c.n, c.ppf, 3)), inverse,
                                        L.stream_ptr()))


def _r2q(L, c, g, o):
    n = g["R"].shape[0]
    L.check(L.lib.mdgen_rot_to_quat(n, L.ptr(g["R"]), L.ptr(o.new("quat", n, 4)), L.stream_ptr()))


def _prep(L, c, g, o):
    D = 28 if c.tps else 21
    sh = L.Shape(c.B, c.T, c.L)
    L.check(L.lib.mdgen_prep_latents(C.byref(sh), c.tps, c.ci, L.ptr(g["rots"]), L.ptr(g["trans"]), L.ptr(g["torsions"]),
                                     L.ptr(o.new("latents", c.B, c.T, c.L, D)), L.ptr(o.new("x_cond", c.B, c.T, c.L, D)),
                                     L.ptr(o.new("x_cond_mask", c.B, c.T, c.L, dtype=torch.int64)), L.stream_ptr()))


def _post(L, c, g, o):
    from mdgen_amd.geometry import residue_tables
    tb = residue_tables(o.dev)
    sh = L.Shape(c.B, c.T, c.L)
    L.check(L.lib.mdgen_samples_to_atom14(C.byref(sh), 28 if c.tps else 21, c.tps, L.ptr(g["samples"]), L.ptr(g["rot0"]), L.ptr(g["trans0"]),
                                          L.ptr(g["seqres"]), L.ptr(tb["default_frames"]), L.ptr(tb["lit_positions"]), L.ptr(tb["atom14_group"]),
                                          L.ptr(tb["atom14_mask"]), L.ptr(o.new("atom14", c.B, c.T, c.L, 14, 3)), L.stream_ptr()))


def _cond(L, c, g, o):
    from mdgen_amd.geometry import residue_tables
    tb = residue_tables(o.dev)
    L.check(L.lib.mdgen_atom14_to_cond(c.B, c.L, L.ptr(g["atom14"]), L.ptr(g["seqres"]), L.ptr(tb["atom37_to_atom14"]), L.ptr(tb["atom37_mask"]),
                                       L.ptr(tb["chi_atom_indices"]), L.ptr(tb["chi_angles_mask"]), L.ptr(o.new("rots", c.B, c.L, 3, 3)),
                                       L.ptr(o.new("trans", c.B, c.L, 3)), L.ptr(o.new("torsions", c.B, c.L, 7, 2)),
                                       L.ptr(o.new("torsion_mask", c.B, c.L, 7)), L.stream_ptr()))


def _plan(L, c, g, o):
    B = len(SR.PLAN_T)
    L.check(L.lib.mdgen_path_plan(B, c.per, c.gvp, L.ptr(g["t"]), L.ptr(g["x0"]), L.ptr(g["x1"]), L.ptr(o.new("xt", B, c.per)),
                                  L.ptr(o.new("ut", B, c.per)), L.stream_ptr()))


def _mse(L, c, g, o):
    for k in SR.MSE_MASKS:
        L.check(L.lib.mdgen_masked_mse(SR.MSE_B, c.per, L.ptr(g["pred"]), L.ptr(g["target"]), L.ptr(g[f"mask_{k}"]),
                                       L.ptr(o.new(f"loss_{k}", SR.MSE_B)), L.stream_ptr()))


_RUN = dict(algebra=_algebra, apply=_apply, r2q=_r2q, prep=_prep, post=_post, cond=_cond, plan=_plan, mse=_mse)


def _device(case, dev):
    import mdgen_amd._lib as L
    inp = SR.reference(case)[0]
    g = {k: v.to(dev).contiguous() for k, v in inp.items()}
    o = _Outputs(dev)
    _RUN[case.group](L, case, g, o)
    out = o.collect()
    out.pop("ident_R", None)
    return out


@pytest.mark.parametrize("case", SR.CASES, ids=[c.id for c in SR.CASES])
def test_se3_kernels_unit(case):
    dev = _cuda()
    out = _device(case, dev)
    got, floor = SR.verify(case, out)
    print(SR.report_line(case.id, got, floor))
    # no atomics on these paths: the same bits from a second call
    again = _device(case, dev)
    for k in out:
        assert torch.equal(out[k].view(torch.int32) if out[k].dtype == torch.float32 else out[k],
                           again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]), (case.id, k)
