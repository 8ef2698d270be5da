"""The fixed-grid Runge-Kutta solvers inside the fused drivers (mdgen_rollout_rk, mdgen_upsample_rk; csrc/ode.inc): the fused
rollout against the chain of inference() + atom14_to_cond block by block, bit for bit, also where a block does not start on 16
bytes; capture and its cache key; the fused upsampling against its three parts; the rollout against the CPU oracle driven block
by block (tests/rk_ref.py); dopri5 through rollout(); and the CLI with and without --per_block."""
import functools

import numpy as np
import pytest
import torch

import rk_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
METHODS = list(R.METHODS)
D = 21


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _setup(B, T, L_, R_, wseed=9, bseed=31, zseed=5):
    """A forward-simulation wrapper built in fp32 mode (it can switch to bf16), its weights, the one-frame conditioning batch of
    `sim_inference.get_batch`'s layout and R_ blocks of noise."""
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_batch, synth_state_dict
    from mdgen_amd.wrapper import NewMDGenWrapper
    dev = _cuda()
    cfg = ModelConfig.forward_sim(num_frames=T, crop=max(L_, 4))
    sd = synth_state_dict(cfg, wseed)
    w = NewMDGenWrapper(cfg, device=dev, precision="fp32")
    w.model.load_state_dict(sd)
    batch = synth_batch(B, 1, L_, 0, dev, seed=bseed)
    zs = torch.randn(R_, B, T, L_, D, generator=torch.Generator().manual_seed(zseed)).to(dev)
    return w, sd, cfg, batch, zs


def _chain(w, batch, T, S, zs, method):
    """R rounds of sim_inference.rollout: inference() + atom14_to_cond per block -> (atom14, samples, next batch)."""
    from mdgen_amd.sim_inference import rollout as py_rollout
    blocks, samples, cur = [], [], dict(batch)
    for z in zs:
        a, cur = py_rollout(w, cur, T, S, zs=z, sampling_method=method)
        blocks.append(a)
        samples.append(w.last_samples.clone())
    return torch.cat(blocks, 1), torch.stack(samples), cur


def _assert_same_rollout(got, want, tag):
    (a, s, nxt), (ca, cs, cur) = got, want
    assert torch.isfinite(a).all() and torch.isfinite(s).all(), tag
    assert torch.equal(a, ca), f"{tag}: atom14"
    assert torch.equal(s, cs), f"{tag}: last_samples"
    for k in ("trans", "rots", "torsions"):
        assert torch.equal(nxt[k], cur[k]), f"{tag}: next {k}"


def _fused(w, batch, T, R_, S, zs, method, use_graph=True):
    a, nxt = w.rollout(batch, T, R_, num_steps=S, zs=zs, sampling_method=method, use_graph=use_graph, return_next=True)
    return a, w.last_samples.clone(), nxt


# ---- 1: the fused rollout is the chain --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("method", METHODS)
def test_fused_rollout_equals_the_chain_bit_for_bit(method, precision):
    B, T, L_, S, R_ = 2, 12, 4, 3, 3
    w, _, _, batch, zs = _setup(B, T, L_, R_)
    w.model.set_precision(precision)
    want = _chain(w, batch, T, S, zs, method)
    got = _fused(w, batch, T, R_, S, zs, method)
    assert got[0].shape == (B, R_ * T, L_, 14, 3) and got[1].shape == (R_, B, T, L_, D)
    assert not torch.equal(got[1], zs)
    _assert_same_rollout(got, want, (method, precision))


# ---- 2: blocks that do not start on 16 bytes --------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["rk4", "midpoint"])
def test_blocks_off_16_bytes(method):
    """315 floats per block: in a contiguous (R, B, T, L, D) tensor blocks 1 and 2 start 12 and 8 bytes past a 16-byte boundary,
    where k_rk_update's 16-byte accesses may not go.  The staged stride is rounded up; the caller sees none of it."""
    B, T, L_, S, R_ = 1, 5, 3, 2, 3
    assert (B * T * L_ * D) % 4 != 0
    w, _, _, batch, zs = _setup(B, T, L_, R_, bseed=33, zseed=7)
    w.model.set_precision("bf16")
    want = _chain(w, batch, T, S, zs, method)
    for use_graph in (False, True, True):
        _assert_same_rollout(_fused(w, batch, T, R_, S, zs, method, use_graph), want, (method, use_graph))


# ---- 3: capture -------------------------------------------------------------------------------------------------------------
def test_rollout_capture_replay_and_key():
    from mdgen_amd.synthetic import synth_batch
    B, T, L_, R_ = 2, 12, 4, 3
    w, _, _, batch, zs = _setup(B, T, L_, R_)
    w.model.set_precision("bf16")
    run = lambda bt, method, S, g: _fused(w, bt, T, R_, S, zs, method, use_graph=g)
    same = lambda x, y: torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and all(torch.equal(x[2][k], y[2][k]) for k in ("trans", "rots", "torsions"))
    first = run(batch, "rk4", 3, True)         # captured
    assert same(first, run(batch, "rk4", 3, True))     # replayed
    assert same(first, run(batch, "rk4", 3, False))
    # another start frame through the same staging buffers and the same graph
    batch2 = synth_batch(B, 1, L_, 0, w.device, seed=77)
    second = run(batch2, "rk4", 3, True)
    assert same(second, run(batch2, "rk4", 3, False)) and not torch.equal(second[0], first[0])
    # method and step count are in the key
    mid = run(batch, "midpoint", 3, True)
    s4 = run(batch, "rk4", 4, True)
    again = run(batch, "rk4", 3, True)
    assert same(again, first)
    assert not torch.equal(mid[1], first[1]) and not torch.equal(s4[1], first[1])
    assert same(mid, run(batch, "midpoint", 3, False)) and same(s4, run(batch, "rk4", 4, False))


def test_rollout_rk_graph_is_keyed_on_every_residue_table():
    """As test_rollout_graph_is_keyed_on_every_residue_table for Euler: a call that differs from a cached one only in
    `lit_positions` captures its own graph.  Graph calls a, b, a: each equals its eager counterpart bit for bit."""
    from mdgen_amd.geometry import residue_tables
    B, T, L_, R_, S = 2, 12, 4, 2, 2
    w, _, _, batch, zs = _setup(B, T, L_, 3)
    w.model.set_precision("bf16")
    zs = zs[:R_].contiguous()
    dev = w.device
    rots, trans, tors = batch["rots"][:, 0].contiguous(), batch["trans"][:, 0].contiguous(), batch["torsions"][:, 0].contiguous()
    mask = torch.ones(B, T, L_, device=dev)
    tables_a = residue_tables(dev)
    tables_b = dict(tables_a)
    tables_b["lit_positions"] = tables_a["lit_positions"] * 1.5

    def run(tables, use_graph):
        return w.model.rollout_rk(zs, "rk4", S, mask, rots, trans, tors, batch["seqres"], tables, use_graph=use_graph)[:2]
    eager_a, eager_b = run(tables_a, False), run(tables_b, False)
    assert torch.isfinite(eager_a[0]).all() and torch.isfinite(eager_b[0]).all()
    assert not torch.equal(eager_a[0], eager_b[0])
    for name, tables, eager in (("a", tables_a, eager_a), ("b", tables_b, eager_b), ("a again", tables_a, eager_a)):
        atom14, samples = run(tables, True)
        assert torch.equal(atom14, eager[0]), f"graph call {name}: atom14 is not the eager call's"
        assert torch.equal(samples, eager[1]), f"graph call {name}: samples are not the eager call's"


# ---- 4: fused upsampling ----------------------------------------------------------------------------------------------------
def _upsample_parts(w, kb, zs, T, c, S, method, use_graph):
    """prep_keyframes -> model.sample_rk -> samples_to_atom14: the fused call's three steps as three calls."""
    from mdgen_amd.geometry import prep_keyframes, samples_to_atom14
    B, _, L_ = kb["trans"].shape[:3]
    p = prep_keyframes(kb["rots"], kb["trans"], kb["torsions"], T, c)
    mask = kb["mask"].float()[:, None].expand(B, T, L_).contiguous()
    samples = w.model.sample_rk(zs, method, S, mask=mask, start_frames=(p["start_rot"], p["start_trans"]), x_cond=p["x_cond"],
                                x_cond_mask=p["x_cond_mask"], aatype=kb["seqres"], use_graph=use_graph)
    return samples_to_atom14(samples, p["start_rot"], p["start_trans"], kb["seqres"], False), samples


@pytest.mark.parametrize("method", METHODS)
def test_fused_upsample_rk_is_the_sum_of_its_parts(method):
    from test_upsampling_gpu import case_2_12_4, key_frames, make_wrapper, to_dev
    dev = _cuda()
    B, T, L_, c, S, kbA, _, zs = case_2_12_4()
    kbB, _ = key_frames(B, T, L_, c, 177)
    w, _, _ = make_wrapper(T, c)
    z = zs.to(dev)
    refs = {tag: _upsample_parts(w, to_dev(kb, dev), z, T, c, S, method, False) for tag, kb in (("A", kbA), ("B", kbB))}
    assert torch.isfinite(refs["A"][0]).all() and not torch.equal(refs["A"][1], refs["B"][1])
    calls = []
    orig = w.model.upsample_rk
    w.model.upsample_rk = lambda *a, **k: (calls.append(k.get("use_graph")), orig(*a, **k))[1]
    # eager, captured, replayed; then new key frames in the same staging buffers through the same graph, and back
    for tag, kb, use_graph in (("A", kbA, False), ("A", kbA, True), ("A", kbA, True), ("B", kbB, True), ("A", kbA, True)):
        a14, aa = w.upsample(to_dev(kb, dev), zs=z, num_steps=S, sampling_method=method, use_graph=use_graph)
        assert a14.shape == (B, T, L_, 14, 3) and aa.shape == (B, T, L_)
        assert torch.equal(w.last_samples, refs[tag][1]), (tag, use_graph)
        assert torch.equal(a14, refs[tag][0]), (tag, use_graph)
    assert calls == [False, True, True, True, True]      # one fused call each


# ---- 5: against the oracle --------------------------------------------------------------------------------------------------
def test_rollout_rk4_fp32_vs_oracle_block_by_block():
    """fp32 mode, rk4, S = 3, two blocks: tests/rk_ref.py drives the CPU oracle's forward per block, the oracle's own rollout glue
    (atom14 -> frames, torsions) makes the next conditioning frame.  Block 0 at the single-solve gates of test_rk_fp32_vs_oracle
    (samples rel-L2 1e-5, atom14 max 1e-3 A); block r, which starts from a frame that carries block r - 1's error on each side,
    at (r + 1) x those -- the rule of test_multi_block_rollout_one_graph.

    One entry of the glue is not the oracle's to give: the pre-omega angle of residue 0.  It is built from the zero padding in
    front of the chain -- two coincident phantom atoms -- so its (sin, cos) is the rounding noise of whichever host evaluates the
    formula (tests/test_oracle_cpu.py::test_ten_chained_blocks_vs_reference, which takes that entry from a recording of its
    fixtures' host for the same reason), its mask is 0, and yet prep_batch copies it into x_cond, where seeded weights read it.
    With the oracle's own noise in that entry block 1 showed samples rel-L2 3.40e-03 and atom14 max 1.90e-01 A: a comparison of
    two hosts' rounding, not of the solver.  As in that test, the one entry is taken from the other side of the comparison -- here
    the device's frame -- and every other value of the frame, masked or not, is the oracle's own; the test asserts that the
    entry is masked and that nothing else of the two frames is further apart than 1e-4.  Measured on an MI355X: block 0 samples
    rel-L2 3.93e-07, atom14 max 2.00e-05 A; block 1 5.11e-07 and 2.48e-05 A; the frames handed to block 1 differ by 1.00 in that
    entry and by at most 2.8e-06 anywhere else."""
    from oracle import mdgen_oracle as O
    from mdgen_amd.geometry import atom14_to_cond
    B, T, L_, S, R_ = 2, 12, 4, 3, 2
    w, sd, cfg, batch, zs = _setup(B, T, L_, 3)
    w.model.set_precision("fp32")
    zs = zs[:R_].contiguous()
    atom14 = w.rollout(batch, T, R_, num_steps=S, zs=zs, sampling_method="rk4").cpu()
    samples = w.last_samples.cpu()
    c = O.cfg_dict(cfg)
    cur = {k: v.cpu() for k, v in batch.items()}
    seqres = cur["seqres"]
    measured = []
    for r in range(R_):
        ob = dict(cur)
        for k in ("torsions", "trans", "rots"):
            ob[k] = cur[k].expand(-1, T, *cur[k].shape[2:])
        prep = O.prep_batch(ob, c)
        mk = prep["model_kwargs"]
        ref = R.solve(lambda t, y: O.forward(sd, c, y, torch.ones(B) * t, **mk), zs[r].cpu(), "rk4", S)
        ref14 = O.postprocess(ref, prep["rigids"], seqres, c)[0]
        e = rel_l2(samples[r], ref)
        d = float((atom14[:, r * T:(r + 1) * T] - ref14).abs().max())
        measured.append((e, d))
        print(f"rk4 S={S} block {r}: samples rel-L2 {e:.2e}, atom14 max {d:.2e} A (gates {(r + 1) * 1e-5:.0e}, {(r + 1) * 1e-3:.0e})")
        glue = {k: v.float().clone() for k, v in O.rollout_glue(ref14[:, -1], seqres).items()}
        # the device's frame at the same boundary: residue 0's pre-omega comes from it, the rest is compared and left alone
        dev_c = {k: v.cpu() for k, v in atom14_to_cond(atom14[:, (r + 1) * T - 1].to(w.device), batch["seqres"]).items()}
        assert (dev_c["torsion_mask"][:, 0, 0] == 0).all()
        dt_ = (dev_c["torsions"] - glue["torsions"][:, 0]).abs().amax(-1)        # (B, L, 7)
        noise = float(dt_[:, 0, 0].max())
        dt_[:, 0, 0] = 0
        rest = max(float(dt_.max()), float((dev_c["rots"] - glue["rots"][:, 0]).abs().max()), float((dev_c["trans"] - glue["trans"][:, 0]).abs().max()))
        print(f"  frame after block {r}, device glue - oracle glue: pre-omega of residue 0 {noise:.2e}, everything else {rest:.2e}")
        assert rest <= 1e-4, (r, rest)
        glue["torsions"][:, 0, 0, 0] = dev_c["torsions"][:, 0, 0]
        cur = dict(cur, **glue)
    for r, (e, d) in enumerate(measured):
        assert e <= (r + 1) * 1e-5 and d <= (r + 1) * 1e-3, (r, e, d)


# ---- 6: dopri5 through rollout() --------------------------------------------------------------------------------------------
def test_rollout_dopri5_is_the_chain_of_inference_calls():
    from mdgen_amd._lib import MdgenError
    B, T, L_, R_ = 2, 12, 4, 2
    w, _, _, batch, zs = _setup(B, T, L_, 3)       # (the shape, weights and seeds of tests/test_ode_gpu.py)
    w.model.set_precision("fp32")
    zs = zs[:R_].contiguous()
    from mdgen_amd.sim_inference import rollout as py_rollout
    blocks, samples, stats, cur = [], [], [], dict(batch)
    for z in zs:
        a, cur = py_rollout(w, cur, T, None, zs=z, sampling_method="dopri5")
        blocks.append(a)
        samples.append(w.last_samples.clone())
        stats.append(w.last_stats)
    got = _fused(w, batch, T, R_, None, zs, "dopri5")
    _assert_same_rollout(got, (torch.cat(blocks, 1), torch.stack(samples), cur), "dopri5")
    assert isinstance(w.last_stats, list) and len(w.last_stats) == R_
    assert [st["nfe"] for st in w.last_stats] == [st["nfe"] for st in stats] and all(st["nfe"] >= 8 for st in stats)
    with pytest.raises(MdgenError, match="dopri5"):
        w.rollout(batch, T, R_, num_steps=4, zs=zs, sampling_method="dopri5")


# ---- 7: the CLI -------------------------------------------------------------------------------------------------------------
def test_sim_inference_cli_fused_equals_per_block(tmp_path, monkeypatch):
    """`--sampling_method rk4` with and without --per_block, same seed: identical .npy files (the fused call draws a block's
    noise as the per-block loop does).  Without --per_block every peptide group is ONE rollout_rk call with use_graph on -- seen
    by a spy on the model-level call, as test_use_graph_flag_reaches_the_library sees sample_euler's; --per_block makes none."""
    import pandas as pd
    from mdgen_amd.geometry import restype_order, samples_to_atom14
    from mdgen_amd.model import LatentMDGenModel
    from mdgen_amd.rigid_utils import Rotation
    from mdgen_amd import sim_inference as cli
    dev = _cuda()
    T, Rn, S = 12, 2, 4
    names = {"FLRH": "FLRH", "AWKD": "AWKD"}
    gen = torch.Generator().manual_seed(5)
    data = tmp_path / "data"
    data.mkdir()
    for n, sq in names.items():
        q = torch.randn(1, 4, 4, generator=gen)
        Rm = Rotation(quats=(q / q.norm(dim=-1, keepdim=True)).to(dev)).get_rot_mats()
        tr_ = torch.cumsum(2.2 * torch.randn(1, 4, 3, generator=gen), 1).to(dev)
        ang = 6.2831853 * torch.rand(1, 4, 7, generator=gen)
        lat = torch.zeros(1, 1, 4, 21, device=dev)
        lat[..., 0] = 1.0
        lat[..., 7:21] = torch.stack([ang.sin(), ang.cos()], -1).reshape(1, 1, 4, 14).to(dev)
        a14 = samples_to_atom14(lat, Rm, tr_, torch.tensor([[restype_order[ch] for ch in sq]], device=dev), tps=False)[0]
        np.save(data / f"{n}.npy", a14.cpu().numpy().repeat(3, 0).astype(np.float16))
    split = tmp_path / "split.csv"
    pd.DataFrame({"name": list(names), "seqres": list(names.values())}).to_csv(split, index=False)
    seen = []
    orig = LatentMDGenModel.rollout_rk

    def spy(self, *a, **k):
        seen.append(k.get("use_graph"))
        return orig(self, *a, **k)
    monkeypatch.setattr(LatentMDGenModel, "rollout_rk", spy)
    outs = {}
    for tag, extra in (("fused", []), ("per_block", ["--per_block"])):
        outs[tag] = tmp_path / tag
        torch.manual_seed(1234)
        res = cli.main(["--synthetic", "--data_dir", str(data), "--split", str(split), "--out_dir", str(outs[tag]), "--num_frames", str(T),
                        "--num_rollouts", str(Rn), "--npy", "--sampling_method", "rk4", "--num_steps", str(S)] + extra)
        assert res["frames"] == len(names) * Rn * T
        assert seen == [True] * len(names)      # one group per peptide (--batch 1); nothing added by the --per_block run
    for n in names:
        a, b = np.load(outs["fused"] / f"{n}.npy"), np.load(outs["per_block"] / f"{n}.npy")
        assert a.shape == (Rn * T, 4, 14, 3) and np.isfinite(a).all() and np.array_equal(a, b), n
