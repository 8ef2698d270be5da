"""The invariant point attention kernels alone (`mdgen_debug_ipa_attention`: k_ipa_attn, k_ipa_attn_tiled, k_ipa_attn_merge,
k32_ipa_bwd_q / _kv / _reduce, k32_ipa_headw_bwd) against tests/ipa_ref.py `core` in fp64 with autograd, on the device's own fp32
inputs, at the cases of ipa_ref.CASES: both forward kernels, every tile and 256-query edge, one-slice and sliced runs with
slices that lie past L, a scratch that cuts the slice count, the sampler's ngroups = steps * B call with its bf16 rows.  The gate
of every quantity is 32 x the error of torch's own fp32 against the same fp64 reference (ipa_ref.reference);
tests/test_ipa_attention_cpu.py shows what those gates catch and that every case runs what its comment says."""
import ctypes as C

import pytest
import torch

import ipa_ref as IR

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GUARD = 4096          # floats behind the scratch that no kernel may touch
_FULL = {}


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch.device("cuda")


def _scratch(case, dev):
    """(buffer of part_floats + GUARD floats, every byte 0xFF) or None; the full-size one is allocated once."""
    if case.scratch is None:
        return None
    if case.scratch == "full":
        if "part" not in _FULL:
            _FULL["part"] = torch.empty(IR.PART_FULL + GUARD, dtype=torch.float32, device=dev)
        buf = _FULL["part"]
    else:
        buf = torch.empty(case.part_floats + GUARD, dtype=torch.float32, device=dev)
    buf.view(torch.uint8).fill_(255)
    return buf


def _run(case, g, dev, dhw0, with_part=True, bf16=False):
    """One call of the hook on NaN-filled outputs -> (outputs on the CPU, slices launched forward / backward)."""
    import mdgen_amd._lib as L
    M = case.ngroups * case.L
    bwd = case.bwd is not None
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    feat, lse = nan(M, 256), nan(M, 4)
    dproj, scr = (nan(M, 672), nan(M * 200)) if bwd else (None, None)
    dhw = dhw0.to(dev).clone() if bwd else None
    fb = torch.full((M, 256), float("nan"), device=dev, dtype=torch.bfloat16) if bf16 else None
    part = _scratch(case, dev) if with_part else None
    nf, nb = C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib.mdgen_debug_ipa_attention(
        L.ptr(g["proj"]), L.ptr(g["rot"]), L.ptr(g["trans"]), L.ptr(g["mask"]), L.ptr(g["head_w"]), case.ngroups, case.B, case.L,
        L.ptr(part), case.part_floats if part is not None else 0, L.ptr(g["dfeat"]) if bwd else None, L.ptr(feat), L.ptr(fb),
        L.ptr(lse), L.ptr(dproj), L.ptr(dhw), L.ptr(scr), C.byref(nf), C.byref(nb), L.stream_ptr()))
    torch.cuda.synchronize()
    if part is not None:
        assert bool((part[-GUARD:].view(torch.int32) == -1).all()), "a kernel wrote behind the scratch"
    out = dict(feat=feat.cpu(), lse=lse.cpu())
    if bwd:
        out.update(dproj=dproj.cpu(), dhw_total=dhw.cpu())
    if bf16:
        out["feat_bf16"] = fb.cpu()
    return out, nf.value, nb.value


@pytest.mark.parametrize("case", IR.CASES, ids=[c.id for c in IR.CASES])
def test_ipa_attention_kernels_unit(case):
    import mdgen_amd._lib as L
    dev = _cuda()
    inp, ref, gate, floor = IR.reference(case)
    bwd = case.bwd is not None
    g = {k: inp[k].to(dev).contiguous() for k in ("proj", "rot", "trans", "mask", "head_w", "dfeat")}
    # d head_w is accumulated into: it starts from random values of the gradient's own size
    dhw0 = (inp["dhw0"].double() * ref["dhead_w"].norm() / 2).float() if bwd else None
    out, nf, nb = _run(case, g, dev, dhw0)
    # the slices launched are the host function's, and what the table's comment claims (test_ipa_attention_cpu.py)
    f, b, t = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib.mdgen_debug_ipa_slices(case.ngroups, case.L, int(case.scratch is not None), case.part_floats, C.byref(f), C.byref(b), C.byref(t)))
    assert (nf, nb) == (f.value, b.value if bwd else 0)
    assert nf == case.fwd[0] and (not bwd or nb == case.bwd[0])
    for k in ("feat", "lse") + (("dproj", "dhw_total") if bwd else ()):
        assert torch.isfinite(out[k]).all(), (case.id, k)
    if bwd:
        out["dhead_w"] = out["dhw_total"].double() - dhw0.double()
    got = IR.metrics(out, ref, inp)
    print(IR.report_line(case.id, got, floor))
    IR.check(case.id, got, gate)
    # no float atomics on these paths: the same bits from a second call
    again, _, _ = _run(case, g, dev, dhw0)
    for k in ("feat", "lse") + (("dproj", "dhw_total") if bwd else ()):
        assert torch.equal(out[k], again[k]), (case.id, k)
    if not bwd:
        # the bf16 rows of the default sampler path (one slice, no scratch) = the fp32 rows of the same launch rounded to bf16,
        # to one bf16 ulp; those fp32 rows pass the gates too
        one, nf1, _ = _run(case, g, dev, None, with_part=False, bf16=True)
        assert nf1 == 1
        IR.check(case.id + " one slice", IR.metrics(one, ref, inp), gate)
        a, r = one["feat_bf16"].float(), one["feat"].bfloat16().float()
        assert torch.isfinite(a).all()
        ulp = torch.ldexp(torch.ones(()), torch.frexp(torch.maximum(a.abs(), r.abs()))[1] - 8)    # 2^(floor(log2 |x|) - 7)
        print(f"  bf16 rows: {int((a != r).sum())} of {a.numel()} differ from the rounded fp32 rows")
        assert bool(((a - r).abs() <= ulp).all())
