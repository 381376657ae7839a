#!/usr/bin/env python3
"""Does the prefix-count table (FMH_PREFIX_COUNTS) pay for itself in real use?

    tools/prefix_payoff.py [SITES [SAMPLES [POPULATIONS]]]        (default 2 000 000 x 2 500 samples = 5 000 haplotypes, 5 populations)

One resident cohort whose populations are contiguous column ranges of equal size.  Timed, wall clock around blocking calls: one pack (planes,
row totals, tiled image and - with the option on - the table) plus the Hudson sweep with all seven per-site tracks of EVERY population pair,
the option off and on alternating, three rounds.  Printed per side: the pack, the sweeps and their sum (best and all rounds), per pair the
route (tiled, table, vectors read) and the sweep's time; then the ratio of the sums and the break-even count: the number of sweeps after
which the table's build time is recovered, from the mean saving per sweep."""
import ctypes as C
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ferromic_amd import _abi, device  # noqa: E402
import bench  # noqa: E402


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 2500
    P = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    H = 2 * N
    lib = _abi.load()
    poc = (np.arange(H) * P // H).astype(np.uint8)
    dm = device.DeviceMatrix.alloc(S, N, 2, with_missing=False, max_allele=1, device=0)
    dm.generate(S + N, 0, bench.synthetic_thresholds(S, 0, S + N), (poc & 1).astype(np.uint8), 0)
    bufs = [device.DeviceBuffer(0, 8 * S) for _ in range(7)]
    sites = _abi.HudsonSites(None, *(b.ptr for b in bufs))
    totals = _abi.HudsonTotals()
    pairs = list(itertools.combinations(range(P), 2))
    res = {"off": [], "on": []}
    routes, fst = {}, {}
    for rnd in range(3):
        for side, value in (("off", "0"), ("on", "1")):
            _abi.set_option("FMH_PREFIX_COUNTS", value)
            t0 = time.perf_counter()
            dm.pack(release_bytes=False)
            t1 = time.perf_counter()
            per_pair = []
            for i, j in pairs:
                g = device.Groups(dm, np.stack([poc == i, poc == j]).astype(np.uint8))
                ta = time.perf_counter()
                _abi.check(lib.fmh_hudson_sweep(dm._h, g._h, 0, S, _abi.FORMULA_DENSE, C.byref(sites), C.byref(totals), None))
                per_pair.append(time.perf_counter() - ta)
                routes[side, i, j] = (device.sweep_tiled(dm, g, device.SWEEP_HUDSON)[0],) + device.sweep_prefix(dm, g, device.SWEEP_HUDSON)[:2]
                fst.setdefault((i, j), []).append(totals.numerator_sum / totals.denominator_sum)
            t2 = time.perf_counter()
            res[side].append({"pack_s": t1 - t0, "sweeps_s": t2 - t1, "sweep_calls_s": sum(per_pair), "total_s": t2 - t0, "per_pair_ms": [round(1e3 * x, 3) for x in per_pair]})
    _abi.set_option("FMH_PREFIX_COUNTS", None)
    # (the two kernels differ in occupancy, hence in their default grids and in the order of the regional f64 sums: the 1e-9 contract)
    worst = max(abs(x - v[0]) / abs(v[0]) for v in fst.values() for x in v)
    assert worst <= 1e-9, f"the two sides disagree on a regional F_ST by {worst}"
    out = {"sites": S, "haplotypes": H, "populations": P, "pairs": len(pairs), "tracks": 7}
    for side in ("off", "on"):
        r = res[side]
        out[side] = {"total_s": [round(x["total_s"], 4) for x in r], "pack_s": [round(x["pack_s"], 4) for x in r], "sweep_calls_s": [round(x["sweep_calls_s"], 4) for x in r],
                     "per_pair_ms_best": [min(x["per_pair_ms"][k] for x in r) for k in range(len(pairs))],
                     "routes": {f"{i}-{j}": {"tiled": routes[side, i, j][0], "table": routes[side, i, j][1], "vectors_read": routes[side, i, j][2]} for i, j in pairs}}
    med = lambda side, key: float(np.median([x[key] for x in res[side]]))  # noqa: E731
    build = med("on", "pack_s") - med("off", "pack_s")
    saving = (med("off", "sweep_calls_s") - med("on", "sweep_calls_s")) / len(pairs)
    out["median_total_on_over_off"] = round(med("on", "total_s") / med("off", "total_s"), 4)
    out["table_build_s"] = round(build, 5)
    out["mean_saving_per_sweep_s"] = round(saving, 6)
    out["break_even_sweeps"] = None if saving <= 0 else round(max(build, 0.0) / saving, 2)
    out["worst_relative_difference_of_a_regional_fst"] = worst
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
