"""CPU: the plans of the training step (`mdgen_debug_train_plan`, host only) against kernel traces, and the row-storage invariant.

`tests/golden/train_plan_kernels.json` holds, per case, how often one step launched each kernel that a plan entry names.  The
counts were read off `rocprofv3 --kernel-trace` runs of the step on an MI355X, taken with the library as it was BEFORE the plans
existed (the launchers then chose their kernel by falling through their own conditions): the table is what the plans must
reproduce, not what they print.  A form is named by its kernel, so plan entry <-> traced kernel is one-to-one; what a name cannot
tell (the sequence-resident attention with or without RoPE inside) shows in the count of `k32_rope` launches.
"""
import collections
import json
import os

import pytest

from mdgen_amd import _lib as L

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_plan_kernels.json")))

# one layer; (B, T, L, two-sided model, bytes every weight is off a 16-byte boundary)
CASES = {
    "B1_T8_L16": (1, 8, 16, False, 0),            # 128 trunk rows: every small form
    "B1_T24_L64": (1, 24, 64, False, 0),          # 1 536 rows: streamed, at most 2 048 rows, no bf16 rows
    "B1_T40_L64": (1, 40, 64, False, 0),          # 2 560 rows: above 2 048, below 4 096
    "B1_T130_L32": (1, 130, 32, False, 0),        # 4 160 rows: bf16 rows; temporal axis sequence-resident, residue axis chunked
    "B8_T2_L160": (8, 2, 160, False, 0),          # 1 280 IPA rows: wide forms with m % 384 != 0; residue axis sequence-resident
    "B1_T130_L32_mis": (1, 130, 32, False, 4),    # ... with the parameter buffer bound 4 bytes off
    "tps_B2_T50_L44": (2, 50, 44, True, 0),
}
LINEAR = ("k32_linear", "k16_linear_wdma<false>", "k16_linear_wdma<true>", "k16_linear_wide", "k16_linear_small", "k16_linear_fast",
          "k16_linear")
DW_WIDE = ("k16_dw_wide<false, false>", "k16_dw_wide<true, false>", "k16_dw_wide<false, true>", "k16_dw_wide<true, true>")
DW_OTHER = ("k32_dw", "k16_dw<true>", "k16_dw<false>")
ATTN = ("k32_attn", "k16_attn", "k16_attn_seq")


def _launches(plan, tps, prec):
    """Kernel -> launches of one step with one layer and every gradient wanted, from the plans alone."""
    n = collections.Counter()
    for block in ["ipa"] * (2 if tps else 1):
        b = plan[block + "_block"]
        for f in b["proj"] + [b["out"]]:
            n[f] += 1
        for k in ("q", "kv", "q_points", "kv_points", "out"):
            n[b["dx_" + k][1]] += 1
            n[b["dw_" + k][0]] += 1
    subs = [plan["ipa_attn"], plan["ipa_mlp"]] * (2 if tps else 1) + [plan["trunk_attn_l"], plan["trunk_attn_t"], plan["trunk_mlp"]]
    for s in subs:
        n[s["gate"]] += 1
        n[s["ln"]] += 1
        if "attn" in s:
            for f in s["qkv"] + [s["out"], s["dx_out"][1]]:
                n[f] += 1
            n[s["dw_out"][0]] += 1
            each = 1 if prec == 16 else 3      # bf16 operands: q | k | v backward as one product; fp32: three layers
            n[s["dx_qkv"][1]] += each
            n[s["dw_qkv"][0]] += each
            n[s["attn"].replace("+rope", "")] += 1
            n["k32_rope"] += 0 if s["attn"].endswith("+rope") else 1
        else:
            for f in (s["fc1"], s["fc2"], s["dx_fc2"][1], s["dx_fc1"][1], s["dw_fc2"][0], s["dw_fc1"][0]):
                n[f] += 1
    f = plan["final"]
    for k in (f["lin"], f["ln"], f["dx"][1], f["dw"][0]):
        n[k] += 1
    return n


@pytest.mark.parametrize("name,prec", [(c, p) for c in CASES for p in (32, 16)], ids=str)
def test_train_plan_matches_the_traced_kernels(name, prec):
    """Every kernel a plan entry names is launched as often as the trace of the step (before the plans existed) shows.  The
    weight gradients outside the sub-layers are planned where they are launched and are a fixed set: three adaLN heads and the time
    embedder's two layers (a handful of rows, every size a multiple of 8: k16_dw<true>), the two token embedders and, two-sided
    model, the two relative-frame embedders (a contraction of 21 / 28 / 7: k16_dw<false>); k32_dw for all with fp32 operands."""
    B, T, L_, tps, mis = CASES[name]
    plan = L.train_plan(B, T, L_, tps=tps, num_layers=1, train_precision=prec, weight_misalign_bytes=mis)
    got = _launches(plan, tps, prec)
    if prec == 32:
        got["k32_dw"] += 9 if tps else 7
    else:
        got["k16_dw<true>"] += 5
        got["k16_dw<false>"] += 4 if tps else 2
    want = GOLDEN[f"{name}/p{prec}"]
    for k in LINEAR + DW_WIDE + DW_OTHER + ATTN + ("k32_gate_bwd_sums", "k32_gate_mul", "k32_ln_bwd_sums", "k32_rope"):
        assert got[k] == want.get(k, 0), (k, got[k], want.get(k, 0))
    assert plan["rows"] == {"ipa": B * L_, "trunk": B * T * L_}


def _dw_rows(form):
    """(X, dY) are read as bf16 rows by this weight-gradient form: the template arguments of the wide kernel."""
    return ("<true" in form and form.startswith("k16_dw_wide"), "true>" in form and form.startswith("k16_dw_wide"))


def _check_rows(s):
    """bf16 rows only where every product that reads them is streamed / wide in the same plan (the launchers refuse anything else
    with -7), and no form that reads bf16 rows without them."""
    bf = s["rows"] == "bf16"
    bf16_rows_in = ["streamed", "k16_linear_wdma<true>"]
    if "attn" in s:
        dq = s["dqkv"] == "bf16"
        assert not dq or (bf and s["attn"].startswith("k16_attn_seq"))
        assert (s["qkv"] == bf16_rows_in[1:]) == bf and (s["dx_out"] == bf16_rows_in) == bf and (s["dx_qkv"] == bf16_rows_in) == dq, s
        assert _dw_rows(s["dw_out"][0]) == (False, bf) and _dw_rows(s["dw_qkv"][0]) == (bf, dq), s
        assert s["out"] != "k16_linear_wdma<true>"            # (the attention output is fp32 always)
    else:
        assert all((s[k] == bf16_rows_in[1]) == bf for k in ("fc1", "fc2")) and all((s[k] == bf16_rows_in) == bf for k in ("dx_fc2", "dx_fc1")), s
        assert _dw_rows(s["dw_fc2"][0]) == (bf, bf) and _dw_rows(s["dw_fc1"][0]) == (bf, bf), s
    assert not bf or s["gate"] == "k32_gate_bwd_sums"      # (the one-pass gate kernel is the one that writes du as bf16 rows)
    for k in ("dw_out", "dw_qkv", "dw_fc2", "dw_fc1"):     # a bias gradient of rows stored as bf16 rides in the wide pass
        assert k not in s or not _dw_rows(s[k][0])[1] or s[k][1], s


SWEEP = [(1, 8, 16), (1, 24, 64), (1, 40, 64), (1, 130, 32), (8, 2, 160), (2, 50, 44), (1, 250, 256), (8, 1000, 4), (1, 32, 128),
         (2, 150, 16), (1, 100, 83)]


@pytest.mark.parametrize("mis", [0, 4, 8], ids=lambda m: f"off{m}")
def test_bf16_rows_only_where_every_consumer_reads_them(mis):
    """The invariant over a sweep of shapes, both model kinds and both precisions; weights off a 16-byte boundary (no streamed
    form can take them) turn the bf16 rows off everywhere; fp32 operands never have them."""
    seen = set()
    for B, T, L_ in SWEEP:
        for tps in (False, True):
            for prec in (32, 16):
                plan = L.train_plan(B, T, L_, tps=tps, num_layers=1, train_precision=prec, weight_misalign_bytes=mis)
                for key in ("ipa_attn", "ipa_mlp", "trunk_attn_l", "trunk_attn_t", "trunk_mlp"):
                    _check_rows(plan[key])
                    if mis or prec == 32:
                        assert plan[key]["rows"] == "fp32" and plan[key].get("dqkv", "fp32") == "fp32", (key, plan[key])
                    seen.add((plan[key]["rows"], plan[key].get("dqkv")))
    if mis == 0:
        assert {("bf16", "bf16"), ("bf16", "fp32"), ("bf16", None), ("fp32", "fp32"), ("fp32", None)} <= seen
