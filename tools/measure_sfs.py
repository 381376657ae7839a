#!/usr/bin/env python3
"""Development measurement of the site frequency spectrum kernel (fmh_sfs, fmh_sfs_joint) beside the EXISTING fmh_population_summaries
sweep of the same group(s) on the same matrix in the same process.  That sweep reads the same planes, writes two u32 tracks per group and
is what a user had to run (and then histogram on the host) before the spectra existed, so it is the yardstick; no ratio is fixed in advance.

Cohort: fmh_matrix_generate, complete and biallelic, allele frequencies skewed to rare alleles (most sites in bins 0, 1 and n, as in a real
cohort - the case the on-chip tile exists for), packed.  Groups: every column, and the two halves of the columns.  Cases:

  * fmh_sfs of every column with 1 window and with 10 000 equal windows, and of one half;
  * fmh_sfs_joint of the two halves (a table of (n/2 + 1)^2 bins: only its corners fit on chip);
  * optionally (--item-rows, --lds-bins) the same under other FMH_SFS_ITEM_ROWS / FMH_SFS_LDS_BINS values.

Per case: the library's HIP-event kernel time (fmh_timing_read) and the wall time of the whole call (which for the spectra includes the
zero-fill of the table and the upload of the item table), best of --repeats after one warm-up, and the same two figures for the summaries
sweep.  Before anything is timed the spectra are checked: every row accounted for, and S equal to the sweep's segregating sites.

Needs a GPU.  One JSON line per case to stdout and to profiles/sfs/measure_sfs.jsonl (or --out).
Default shape: 10 000 000 sites x 5 000 haplotypes; `tools/measure_sfs.py 1000000x5000` for others."""
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


def device_cohort(sites, n, seed):
    rng = np.random.default_rng(seed)
    freq = rng.beta(0.2, 2.0, size=sites)
    freq[rng.random(sites) < 0.02] = 1.0  # fixed sites: bin n
    thr = (np.clip(freq, 0.0, 1.0) * float(1 << 24)).astype(np.uint32)[None, :]
    dm = device.DeviceMatrix.alloc(sites, n // 2, 2, False, 1)
    dm.generate(seed, 0, thr, np.zeros(n, dtype=np.uint8), 0)
    dm.pack(release_bytes=True)
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
    ap.add_argument("--windows", type=int, default=10_000)
    ap.add_argument("--item-rows", default="", help="comma-separated FMH_SFS_ITEM_ROWS values to time besides the default")
    ap.add_argument("--lds-bins", default="", help="comma-separated FMH_SFS_LDS_BINS values to time besides the default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfs", "measure_sfs.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(10_000_000, 5000)]
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
            dm = device_cohort(sites, n, seed=sites + n)
            everyone = np.ones((1, n), dtype=np.uint8)
            first = np.zeros((1, n), dtype=np.uint8)
            first[0, : n // 2] = 1
            groups = {"all": device.Groups(dm, everyone), "half": device.Groups(dm, first),
                      "halves": device.Groups(dm, np.concatenate([first, 1 - first]))}
            edges = np.linspace(0, sites, args.windows + 1).astype(np.uint64)
            many = np.stack([edges[:-1], edges[1:]], axis=1)
            plane_bytes = sites * ((n + 127) // 128 * 16)

            # ---- checks before timing
            whole = device.sfs(dm, groups["all"])
            summary = device.population_summaries(dm, groups["all"], want_sites=False).totals[0]
            stats = device.sfs_stats(whole.counts[0])
            windowed = device.sfs(dm, groups["all"], many)
            joint = device.sfs_joint(dm, groups["halves"])
            half = device.sfs(dm, groups["half"])
            ok = (int(whole.counts.sum()) + int(whole.multiallelic[0]) + int(whole.incomplete[0]) == sites
                  and stats["segregating_sites"] == summary["segregating_sites"]
                  and np.array_equal(windowed.counts.sum(axis=0), whole.counts[0])
                  and np.array_equal(joint.counts.sum(axis=1), half.counts[0]))
            del windowed, joint

            # ---- the yardstick: the summaries sweep with its per-site tracks, same groups, same matrix
            yard = {}
            for name in ("all", "half", "halves"):
                g = groups[name]
                tracks = [device.DeviceBuffer(dm.device, 4 * g.n_groups * sites) for _ in range(2)]
                totals = (_abi.PopTotals * g.n_groups)()
                yard[name] = timed(lambda: _abi.check(lib.fmh_population_summaries(dm._h, g._h, 0, sites, device.FORMULA_SUMMARY, tracks[0].ptr,
                                                                                   tracks[1].ptr, totals, None)), args.repeats)
                for t in tracks:
                    t.free()

            def sfs_case(label, group, windows, joint=False):
                g = groups[group]
                w = np.ascontiguousarray(windows, dtype=np.uint64)
                bins = (g.sizes[0] + 1) * ((g.sizes[1] + 1) if joint else 1)
                table = device.DeviceBuffer(dm.device, 8 * bins * len(w))
                if joint:
                    call = lambda: _abi.check(lib.fmh_sfs_joint(dm._h, g._h, 0, sites, table.ptr, None, None))  # noqa: E731
                else:
                    call = lambda: _abi.check(lib.fmh_sfs(dm._h, g._h, w.ctypes.data_as(C.c_void_p), len(w), table.ptr, None, None))  # noqa: E731
                kernel, wall = timed(call, args.repeats)
                table.free()
                emit({"case": f"{sites}x{n} {label}", "sites": sites, "haplotypes": n, "group": group, "windows": len(w), "table_bins": bins * len(w),
                      "checks_pass": bool(ok), "item_rows": _abi.get_option("FMH_SFS_ITEM_ROWS") or device.SFS_DEFAULT_ITEM_ROWS,
                      "lds_bins_cap": _abi.get_option("FMH_SFS_LDS_BINS") or device.SFS_DEFAULT_LDS_BINS, "sfs_kernel_ms": kernel, "sfs_call_wall_ms": wall,
                      "plane0_gb_per_s_at_kernel_ms": plane_bytes / (kernel * 1e-3) / 1e9, "summaries_kernel_ms": yard[group][0],
                      "summaries_call_wall_ms": yard[group][1], "sfs_kernel_over_summaries_kernel": kernel / yard[group][0]})

            one = [(0, sites)]
            sfs_case("sfs 1 window, all columns", "all", one)
            sfs_case(f"sfs {args.windows} windows, all columns", "all", many)
            sfs_case("sfs 1 window, half of the columns", "half", one)
            sfs_case("joint sfs of the two halves", "halves", one, joint=True)
            for value in [v for v in args.item_rows.split(",") if v]:
                with _abi.options(FMH_SFS_ITEM_ROWS=value):
                    sfs_case(f"sfs 1 window, all columns, item rows {value}", "all", one)
                    sfs_case("joint sfs of the two halves, item rows " + value, "halves", one, joint=True)
            for value in [v for v in args.lds_bins.split(",") if v]:
                with _abi.options(FMH_SFS_LDS_BINS=value):
                    sfs_case(f"sfs 1 window, all columns, tile cap {value}", "all", one)
                    sfs_case("joint sfs of the two halves, tile cap " + value, "halves", one, joint=True)
            for g in groups.values():
                g.close()
            dm.close()


if __name__ == "__main__":
    main()
