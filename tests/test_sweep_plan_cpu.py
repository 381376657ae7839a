"""The sweep plan (ferromic_amd/csrc/sweep_plan.hpp) against a recorded table, on the CPU.

`make plan_check` builds sweep_plan_check: plan_sweep() over a fixed list of host-built matrix and group handles - layouts, allele ranges,
called plane, row widths, group counts and geometries, every mode, every routing option at each forcing value, both sets of LDS figures,
an empty row range - one line per case with every field of the plan.  tests/sweep_plans.tsv holds what the decision code answered before
it was gathered into the plan (the bodies of enqueue_sweep, sweep_window, flat_route_taken, tiled_route_taken, wc_kernel_groups,
wc_fused_lane_totals and summaries_single_sweep as they stood, run over the same list): a route, a window, a batch depth, an LDS size or
a refusal that moves shows up here as one differing line, without a GPU."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_match_the_recorded_table():
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), "plan_check"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    run = subprocess.run([os.path.join(ROOT, "ferromic_amd", "bin", "sweep_plan_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "sweep_plans.tsv")) as fh:
        want = fh.read().splitlines()
    assert len(want) > 1000
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  got      {g}\n  expected {w}"
    assert len(got) == len(want), (len(got), len(want))
