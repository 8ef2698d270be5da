"""bench.py's command line: a plain run takes no leg beyond the headline's own steps, `--full` takes the ones that were the
default before (roofline of the dominant kernel, CPU baseline, extra legs), and the `--no-*` options take single ones out."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

HEADLINE = "tetrapeptide_fwdsim_crop4_T1000_B16"
SMALL = "tetrapeptide_fwdsim_crop4_T100_B1"


def _legs(*argv, rank=0, world=1):
    import bench
    return bench.legs_after_timing(bench.build_parser().parse_args(list(argv)), rank, world)


def test_plain_run_takes_no_leg_after_the_timed_steps():
    assert _legs("--gpus", "1", "--steps", "20", "--warmup", "5") == set()
    assert _legs() == set()
    assert _legs("--dump-outputs", "somewhere") == set()
    # the options that used to take single legs out of the default run are still accepted, and change nothing here
    assert _legs("--no-extra", "--no-cpu-baseline", "--no-roofline") == set()
    for wl in (SMALL, "atlas_crop256_T250_B1"):
        assert _legs("--workload", wl) == set()
    assert _legs("--gpus", "8", rank=0, world=8) == set()


def test_full_takes_the_legs_of_the_former_default_run():
    assert _legs("--full") == {"roofline", "cpu_baseline", "extra"}
    assert _legs("--full", "--no-extra") == {"roofline", "cpu_baseline"}
    assert _legs("--full", "--no-cpu-baseline") == {"roofline", "extra"}
    assert _legs("--full", "--no-roofline") == {"cpu_baseline", "extra"}
    assert _legs("--full", "--no-extra", "--no-cpu-baseline", "--no-roofline") == set()
    # the extra legs belong to the headline workload in bf16; another workload or precision keeps its own roofline and CPU baseline
    assert _legs("--full", "--workload", SMALL) == {"roofline", "cpu_baseline"}
    assert _legs("--full", "--precision", "fp32") == {"roofline", "cpu_baseline"}
    # several ranks: rank 0 profiles its own step, nobody runs the one-process legs
    assert _legs("--full", "--gpus", "8", rank=0, world=8) == {"roofline"}
    assert _legs("--full", "--gpus", "8", rank=3, world=8) == set()


def test_full_is_off_by_default_and_changes_no_other_argument():
    import bench
    p = bench.build_parser()
    plain, full = vars(p.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])), vars(p.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"]))
    assert plain.pop("full") is False and full.pop("full") is True
    assert plain == full and plain["steps"] == 7 and plain["warmup"] == 2 and plain["workload"] == HEADLINE


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_line_of_a_small_workload(full, tmp_path):
    """The benchmark as a process on its smallest workload (B 1 x T 100 x L 4, 3 Euler steps, one warm-up and two timed steps): the
    headline fields are there either way and `ms_per_step` and `value` agree with each other; a plain run leaves `roofline`,
    `cpu_baseline` and `extra` null, `--full` fills the first two (the extra legs belong to the headline workload).  Both write the
    same three arrays with `--dump-outputs`."""
    import numpy as np
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", SMALL,
           "--euler-steps", "3", "--dump-outputs", str(out)] + (["--full"] if full else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "sampled MD frames/sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["config"]["workload"] == SMALL
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1 * 100 / (d["ms_per_step"] * 1e-3)) <= 2e-3 * d["value"]   # (both rounded)
    assert d["extra"] is None
    if full:
        assert d["roofline"]["kernel"] and d["roofline"]["avg_launch_ms"] > 0 and d["cpu_baseline"]["value"] > 0
    else:
        assert d["roofline"] is None and d["cpu_baseline"] is None
    shapes = {n: np.load(out / (n + ".npy")).shape for n in ("atom14", "aa_out", "samples")}
    assert shapes["atom14"] == (1, 100, 4, 14, 3) and shapes["samples"][:3] == (1, 100, 4), shapes
    assert all(np.isfinite(np.load(out / (n + ".npy"))).all() for n in shapes)
