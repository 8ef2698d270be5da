"""Host-only checks of the fixed-grid Runge-Kutta drivers (mdgen_rollout_rk, mdgen_upsample_rk; csrc/ode.inc): the two symbols in
the header, the library and `_lib.EXPORTS`; the refusals the library decides before any device call, through ctypes with fake
non-null pointers; and which calls `sim_inference.sample_group` makes for a named solver, with and without --per_block."""
import argparse
import ctypes as C
import os
import re

import torch

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mdgen_rollout_rk", "mdgen_upsample_rk")
B, T, L_, D = 1, 8, 4, 21
BLK = B * T * L_ * D          # 672 floats, a multiple of 4


# ---- 1: the symbols -----------------------------------------------------------------------------------------------------------
def test_header_library_and_exports_have_the_two_entry_points():
    from mdgen_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "mdgen_amd.h")).read()
    for n in NEW:
        assert re.search(r"^int32_t " + n + r"\(mdgen_ctx\* ctx, const mdgen_shape\* shape, int32_t method, int32_t n_steps,", hdr, re.M), n
        assert hasattr(L.lib, n), n
        assert L.EXPORTS.count(n) == 1, n
    # the rule a caller has to know is stated where the entry point is declared
    doc = hdr[:hdr.index("int32_t mdgen_rollout_rk(")]
    doc = doc[doc.rindex("/*"):]
    assert "zs_block_stride" in doc and "multiple of 4" in doc and "16-byte aligned" in doc
    assert "int64_t zs_block_stride" in hdr


# ---- 2: refusals --------------------------------------------------------------------------------------------------------------
FAKE = 4096     # never followed: every refusal below is decided first


def _tables(L, missing=None):
    return L.ResidueTables(*[None if n == missing else FAKE for n, _ in L.ResidueTables._fields_])


ROLLOUT_PTRS = ("zs", "mask", "cond_rots", "cond_trans", "cond_torsions", "seqres", "x_cond", "x_cond_mask", "atom14", "workspace")
UPSAMPLE_PTRS = ("zs", "mask", "key_rots", "key_trans", "key_torsions", "seqres", "x_cond", "x_cond_mask", "start_rot", "start_trans",
                 "atom14", "workspace")


def _rollout(L, method=3, S=4, R=2, stride=BLK, tables=True, tb=None, **over):
    p = {n: FAKE for n in ROLLOUT_PTRS}
    p.update(over)
    sh = L.Shape(B, T, L_)
    tb = tb or _tables(L)
    return L.lib.mdgen_rollout_rk(None, C.byref(sh), method, S, R, p["zs"], stride, p["mask"], p["cond_rots"], p["cond_trans"],
                                  p["cond_torsions"], p["seqres"], p["x_cond"], p["x_cond_mask"], C.byref(tb) if tables else None,
                                  p["atom14"], p["workspace"], 1 << 30, 0, None)


def _upsample(L, method=3, S=4, c=4, tables=True, tb=None, **over):
    p = {n: FAKE for n in UPSAMPLE_PTRS}
    p.update(over)
    sh = L.Shape(B, T, L_)
    tb = tb or _tables(L)
    return L.lib.mdgen_upsample_rk(None, C.byref(sh), method, S, c, p["zs"], p["mask"], p["key_rots"], p["key_trans"],
                                   p["key_torsions"], p["seqres"], p["x_cond"], p["x_cond_mask"], p["start_rot"], p["start_trans"],
                                   C.byref(tb) if tables else None, p["atom14"], p["workspace"], 1 << 30, 0, None)


def test_null_pointers_are_refused():
    from mdgen_amd import _lib as L
    for n in ROLLOUT_PTRS:
        assert _rollout(L, **{n: None}) == -1, n
    for n in UPSAMPLE_PTRS:
        assert _upsample(L, **{n: None}) == -1, n
    assert _rollout(L, tables=False) == -1 and _upsample(L, tables=False) == -1
    for n, _ in L.ResidueTables._fields_:
        assert _rollout(L, tb=_tables(L, n)) == -1, n
    for n in ("default_frames", "lit_positions", "atom14_group", "atom14_mask"):   # (the tables the upsampling tail reads)
        assert _upsample(L, tb=_tables(L, n)) == -1, n
    # with everything else in order the null context is what is left to refuse
    assert _rollout(L) == -1 and _upsample(L) == -1
    assert b"null" in L.lib.mdgen_last_error()


def test_method_steps_blocks_and_interval_are_judged_without_a_context():
    from mdgen_amd import _lib as L
    for f in (_rollout, _upsample):
        for method, S in ((0, 4), (4, 4), (3, 0)):
            assert f(L, method=method, S=S) == -2, (f.__name__, method, S, L.lib.mdgen_last_error())
    assert _rollout(L, R=0) == -2 and b"n_blocks" in L.lib.mdgen_last_error()
    assert _upsample(L, c=0) == -2 and b"cond_interval" in L.lib.mdgen_last_error()


def test_stride_and_alignment_are_refused():
    from mdgen_amd import _lib as L
    assert BLK % 4 == 0
    assert _rollout(L, stride=BLK - 4) == -7 and b"below one block" in L.lib.mdgen_last_error()
    assert _rollout(L, stride=BLK + 2) == -7 and b"multiple of 4" in L.lib.mdgen_last_error()
    assert _rollout(L, zs=FAKE + 8) == -7 and b"16-byte" in L.lib.mdgen_last_error()
    assert _rollout(L, zs=FAKE + 4, stride=BLK + 4) == -7
    assert _upsample(L, zs=FAKE + 8) == -7 and b"16-byte" in L.lib.mdgen_last_error()
    # a padded stride and an aligned pointer pass these checks (the null context is refused next)
    assert _rollout(L, stride=BLK + 4) == -1


# ---- 3: sample_group routing --------------------------------------------------------------------------------------------------
class _Recorder:
    """A model whose rollout() knows the solver keyword."""
    def __init__(self):
        self.calls = []

    def rollout(self, batch, num_frames, num_rollouts, num_steps=None, sampling_method=None):
        self.calls.append(("rollout", num_frames, num_rollouts, num_steps, sampling_method))
        return torch.zeros(1, num_rollouts * num_frames, 4, 14, 3)

    def inference(self, batch, zs=None, num_steps=None, sampling_method=None):
        self.calls.append(("inference", num_steps, sampling_method))
        Tn = batch["trans"].shape[1]
        return torch.zeros(1, Tn, 4, 14, 3), None


class _OldRollout(_Recorder):
    """... and one whose rollout() predates it."""
    def rollout(self, batch, num_frames, num_rollouts, num_steps=None):
        self.calls.append(("rollout", num_frames, num_rollouts, num_steps))
        return torch.zeros(1, num_rollouts * num_frames, 4, 14, 3)


def _args(**kw):
    return argparse.Namespace(**dict(dict(num_frames=6, num_rollouts=3, num_steps=4, sampling_method=None, per_block=False), **kw))


def _batch():
    return {"torsions": torch.zeros(1, 1, 4, 7, 2), "trans": torch.zeros(1, 1, 4, 3), "rots": torch.eye(3).expand(1, 1, 4, 3, 3),
            "seqres": torch.zeros(1, 4, dtype=torch.long), "mask": torch.ones(1, 4)}


def test_sample_group_routes_a_named_solver_through_one_rollout(monkeypatch):
    from mdgen_amd import geometry, sim_inference as cli
    m = _Recorder()
    out = cli.sample_group(m, _batch(), _args(sampling_method="rk4"))
    assert m.calls == [("rollout", 6, 3, 4, "rk4")] and out.shape[1] == 18
    # --per_block: R inference() calls (the glue between them is the device's; a stand-in here)
    monkeypatch.setattr(geometry, "atom14_to_cond", lambda a, s: {"trans": torch.zeros(1, 4, 3), "rots": torch.eye(3).expand(1, 4, 3, 3),
                                                                   "torsions": torch.zeros(1, 4, 7, 2)})
    m = _Recorder()
    out = cli.sample_group(m, _batch(), _args(sampling_method="rk4", per_block=True))
    assert m.calls == [("inference", 4, "rk4")] * 3 and out.shape[1] == 18
    # no solver named: rollout() is called without the keyword
    m = _OldRollout()
    out = cli.sample_group(m, _batch(), _args())
    assert m.calls == [("rollout", 6, 3, 4)] and out.shape[1] == 18
