#!/usr/bin/env python3
"""Development measurement of the haplotype homozygosity kernel (fmh_haplotype_windows).  Nothing existing computes this, so there is no
yardstick and no time is promised: the figures go into DESIGN.md section 3.13 and choose the default of FMH_HAP_THREADS.

Cohort: fmh_matrix_generate, complete and biallelic, packed; the columns are independent draws, so there is no linkage and how long a window
keeps refining depends only on the allele frequencies.  Two cohorts bracket that:
  * "skewed": frequencies beta(0.2, 2.0) as tools/measure_sfs.py - every haplotype is its own class after a few dozen rows and the window
    stops refining there (K == n), so a window costs about the same whatever its length;
  * "rare": every site at frequency 2e-4 - about one carrier per row among 5 000 haplotypes, K grows by about one per row and stays far below
    n over 400 rows, so every row of a window is refined: the cost of a refinement step per row.
Groups: every column, and the first half of the columns.  Windows: --window-rows rows at step --window-rows and at a quarter of it, and one
single window over every row.  Swept: FMH_HAP_THREADS (64, 256, 512, 1024) and FMH_GRID_PER_CU (the default and 1, 2, 4) on the windowed cases,
FMH_HAP_THREADS on the single window; each with and without the partition (d_first).

Per case: the library's HIP-event kernel time (fmh_timing_read) and the wall time of the whole call, best of --repeats after one warm-up.
Before anything is timed every window is checked (sum(top) <= n, distinct >= 1) and the windows inside the first --check-rows rows are
compared with the numpy oracle (tests/hap_ref.py) on a second, small matrix generated with the same seed.

Needs a GPU.  One JSON line per case to stdout and to profiles/haplotypes/measure_haplotypes.jsonl (or --out).
Default shape: 1 000 000 sites x 5 000 haplotypes; `tools/measure_haplotypes.py 200000x5000` for others."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ferromic_amd import _abi, device  # noqa: E402
from tests import hap_ref  # noqa: E402


def thresholds(kind, sites, seed):
    rng = np.random.default_rng(seed)
    freq = rng.beta(0.2, 2.0, size=sites) if kind == "skewed" else np.full(sites, 2e-4)
    return (np.clip(freq, 0.0, 1.0) * float(1 << 24)).astype(np.uint32)[None, :]


def device_cohort(thr, sites, n, seed, keep_bytes=False):
    dm = device.DeviceMatrix.alloc(sites, n // 2, 2, False, 1)
    dm.generate(seed, 0, thr[:, :sites], np.zeros(n, dtype=np.uint8), 0)
    dm.pack(release_bytes=not keep_bytes)
    return dm


def timed(call, repeats):
    """(best kernel ms by the library's events, best wall ms of the call) after one warm-up"""
    lib = _abi.load()
    best_kernel = best_wall = None
    for i in range(repeats + 1):
        _abi.check(lib.fmh_timing_reset())
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        total, launches = C.c_double(), C.c_uint64()
        _abi.check(lib.fmh_timing_read(C.byref(total), C.byref(launches)))
        if i:
            best_kernel = total.value if best_kernel is None else min(best_kernel, total.value)
            best_wall = wall if best_wall is None else min(best_wall, wall)
    return best_kernel, best_wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-rows", type=int, default=400)
    ap.add_argument("--check-rows", type=int, default=2000)
    ap.add_argument("--cohorts", default="skewed,rare")
    ap.add_argument("--threads", default="64,256,512,1024", help="FMH_HAP_THREADS values to time besides the default")
    ap.add_argument("--per-cu", default="1,2,4", help="FMH_GRID_PER_CU values to time besides the default")
    ap.add_argument("--single-window-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotypes", "measure_haplotypes.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 5000)]
    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:

        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for sites, n in shapes:
            for kind in [k for k in args.cohorts.split(",") if k]:
                seed = sites + n
                thr = thresholds(kind, sites, seed)
                dm = device_cohort(thr, sites, n, seed)
                masks = {"all": np.ones(n, dtype=np.uint8), "first-half": np.concatenate([np.ones(n // 2, dtype=np.uint8), np.zeros(n - n // 2, dtype=np.uint8)])}
                groups = {name: device.Groups(dm, mask[None, :]) for name, mask in masks.items()}
                rows = args.window_rows

                def stepped(step):
                    begin = np.arange(0, sites - rows + 1, step, dtype=np.uint64)
                    return np.stack([begin, begin + np.uint64(rows)], axis=1)

                window_sets = {f"{rows} rows at step {rows}": stepped(rows), f"{rows} rows at step {rows // 4}": stepped(rows // 4),
                               "one window, every row": np.array([[0, sites]], dtype=np.uint64)}

                # ---- checks before timing: invariants of every window, and the windows of a prefix against the oracle
                check_rows = min(args.check_rows, sites)
                small = device_cohort(thr, check_rows, n, seed, keep_bytes=True)
                x = small.download()[0].reshape(check_rows, n)
                small.close()
                ok = True
                for name, g in groups.items():
                    for label, w in window_sets.items():
                        got = device.haplotype_windows(dm, g, w, partition=False)
                        size = g.sizes[0]
                        ok = ok and bool((got.top.astype(np.uint64).sum(axis=1) <= size).all() and (got.distinct >= 1).all())
                        inside = w[:, 1] <= check_rows
                        if inside.any():
                            ref = hap_ref.windows(x, None, masks[name].astype(bool), [(int(b), int(e)) for b, e in w[inside]])
                            ok = ok and np.array_equal(got.sum_sq[inside], ref["sum_sq"]) and np.array_equal(got.distinct[inside], ref["distinct"])
                            ok = ok and np.array_equal(got.top[inside], ref["top"])
                        emit({"case": f"{sites}x{n} {kind} check: {name}, {label}", "windows": int(len(w)), "windows_checked_against_oracle": int(inside.sum()),
                              "checks_pass_so_far": bool(ok), "distinct_min_median_max": [int(got.distinct.min()), float(np.median(got.distinct)), int(got.distinct.max())]})

                def case(group, label, w, partition, repeats):
                    g = groups[group]
                    size = g.sizes[0]
                    d_out = device.DeviceBuffer(dm.device, 24 * len(w))
                    d_first = device.DeviceBuffer(dm.device, 4 * size * len(w)) if partition else None
                    call = lambda: _abi.check(lib.fmh_haplotype_windows(dm._h, g._h, w.ctypes.data_as(C.c_void_p), len(w), d_out.ptr,  # noqa: E731
                                                                        d_first.ptr if partition else None, None))
                    kernel, wall = timed(call, repeats)
                    d_out.free()
                    if d_first is not None:
                        d_first.free()
                    window_rows = int((w[:, 1] - w[:, 0]).sum())
                    emit({"case": f"{sites}x{n} {kind}: {group}, {label}", "cohort": kind, "sites": sites, "haplotypes": n, "group": group, "members": size,
                          "windows": int(len(w)), "window_rows_total": window_rows, "partition": bool(partition), "checks_pass": bool(ok),
                          "hap_threads": _abi.get_option("FMH_HAP_THREADS"), "grid_per_cu": _abi.get_option("FMH_GRID_PER_CU"),
                          "kernel_ms": kernel, "call_wall_ms": wall, "kernel_us_per_window": kernel * 1e3 / len(w)})

                thread_values = [None] + [int(v) for v in args.threads.split(",") if v]
                per_cu_values = [None] + [int(v) for v in args.per_cu.split(",") if v]
                for group in groups:
                    for label, w in window_sets.items():
                        single = len(w) == 1
                        repeats = args.single_window_repeats if single else args.repeats
                        for threads in thread_values:
                            for per_cu in ([None] if single else per_cu_values):
                                if threads is not None and per_cu is not None:
                                    continue  # one switch at a time
                                opts = {}
                                if threads is not None:
                                    opts["FMH_HAP_THREADS"] = threads
                                if per_cu is not None:
                                    opts["FMH_GRID_PER_CU"] = per_cu
                                with _abi.options(**opts):
                                    case(group, label, w, False, repeats)
                                    if threads is None or not single:
                                        case(group, label, w, True, repeats)
                for g in groups.values():
                    g.close()
                dm.close()


if __name__ == "__main__":
    main()
