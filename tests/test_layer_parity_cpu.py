"""CPU self-test of tests/layer_parity.py: the per-layer, per-row metric on a stand-in device.

The stand-in is the oracle itself with its 2-D weights rounded to bf16 as the device rounds them (not the fp32 embedding).  (a) Clean, it stays
under the GPU gates.  (b) Two faults the whole-tensor gate (rel-L2 < 1e-2 of out and h_nl against the fp32 oracle) lets through
are caught by the per-layer gate with a margin of >= 10x: the residue-axis attention of every trunk layer attending to padded keys
as if they were real, and 48 of 384 output channels of the temporal attention zeroed for one 64-query block of sample 0.
"""
import pytest
import torch

import layer_parity as LP
from conftest import rel_l2
from oracle import mdgen_oracle as O

torch.set_grad_enabled(False)


def _case(B, T, L, n_pad, data_seed=1, weights_seed=5):
    from mdgen_amd.config import ModelConfig
    from mdgen_amd.synthetic import synth_forward_inputs, synth_state_dict
    cfg = ModelConfig.forward_sim(num_frames=T, crop=max(L, 4))
    sd = synth_state_dict(cfg, weights_seed)
    inp = synth_forward_inputs(cfg, B, T, L, n_pad, data_seed)
    kw = dict(x=inp["x"], t=inp["t"], mask=inp["mask"], start_frames=(inp["start_rot"], inp["start_trans"]),
              end_frames=(inp["end_rot"], inp["end_trans"]), x_cond=inp["x_cond"], x_cond_mask=inp["x_cond_mask"],
              aatype=inp["aatype"])
    return cfg, sd, kw


def _standin(sd, cfg, kw):
    """The oracle with the device's bf16 weight operands: every 2-D weight but the embedding's (the library embeds in fp32)."""
    fp32 = ("latent_to_emb", "cond_to_emb", "mask_to_emb", "aatype_to_emb", "pos_embed")
    sdb = {k: (v.bfloat16().float() if v.dim() == 2 and not k.startswith(fp32) else v) for k, v in sd.items()}
    return O.forward(sdb, O.cfg_dict(cfg), return_trace=True, **kw)


def _padded_keys_attended(real):
    def f(P, pre, y, mask, heads):
        if pre.startswith("layers.") and ".mha_l." in pre:
            mask = torch.ones_like(mask)
        return real(P, pre, y, mask, heads)
    return f


def _channels_zeroed(real, L, q0=512, c0=96, nq=64, nc=48):
    def f(P, pre, y, mask, heads):
        o = real(P, pre, y, mask, heads)
        if pre.startswith("layers.") and ".mha_t." in pre:
            o = o.clone()
            o[:L, q0:q0 + nq, c0:c0 + nc] = 0      # sequences 0 .. L-1 are sample 0's residues
        return o
    return f


@pytest.mark.parametrize("fault, shape", [(None, (2, 70, 9, 2)), ("padded keys attended", (1, 130, 9, 1)),
                                          ("channels zeroed", (2, 1000, 4, 0))], ids=["clean", "padded_keys", "channels"])
def test_per_layer_gate_catches_what_the_whole_tensor_gate_passes(fault, shape, monkeypatch):
    B, T, L, n_pad = shape
    cfg, sd, kw = _case(B, T, L, n_pad)
    ref, rtr = O.forward(sd, O.cfg_dict(cfg), return_trace=True, **kw)
    with monkeypatch.context() as mp:
        if fault == "padded keys attended":
            mp.setattr(O, "mha_rope", _padded_keys_attended(O.mha_rope))
        elif fault == "channels zeroed":
            mp.setattr(O, "mha_rope", _channels_zeroed(O.mha_rope, L))
        out, tr = _standin(sd, cfg, kw)
    nl = cfg.num_layers
    whole = {"out": rel_l2(out, ref), f"h{nl}": rel_l2(tr[f"h{nl}"], rtr[f"h{nl}"])}
    rep = LP.forward_stages(cfg, sd, kw, out, tr, layers=range(nl))
    print(fault or "clean", shape, {k: f"{v:.2e}" for k, v in whole.items()})
    print(LP.report_line(str(shape), rep))
    assert all(v < 1e-2 for v in whole.values()), whole          # the old gate passes the stand-in, with or without the fault
    if fault is None:
        LP.check("clean stand-in", rep)
        return
    gate = LP.GATES["trunk"][0]
    for i in range(nl):
        assert rep[f"layer{i}"]["max"] > 10 * gate, (fault, i, rep[f"layer{i}"]["max"], gate)
    for k in ("ipa", "embed", "final"):                            # the faults sit in the trunk: the other stages stay clean
        assert rep[k]["max"] < LP.GATES[k][0], (k, rep[k]["max"])
