#!/usr/bin/env python3
"""Development measurement of the extended haplotype homozygosity scan (fmh_ehh_scan) against the haplotype window kernel
(fmh_haplotype_windows) in ONE process on the same cohort.  The existing kernel is the yardstick: both refine the same number of rows with
the same step, the scan adds a recount of the pair counts after every row that split a class.  Nothing is promised; the figures go into
DESIGN.md section 3.14 and choose the default of FMH_HAP_THREADS for the scan.

Cohort: section 3.13's "rare" one - fmh_matrix_generate, complete and biallelic, every site at frequency 2e-4 (about one carrier per row among
5 000 haplotypes), packed.  The carriers of a focal row are one or two members, so core 1 holds no pair or one; core 0 is everyone else, K
grows by about one per row and nothing stops early without a threshold: every row up to max_extent is refined, and nearly every row splits
a class (the worst case for the recount).  A second cohort, "monomorphic" (no carrier anywhere), splits nothing: the same rows are walked
with K = 1 and no recount, which tells the cost of the recounts from that of the rest.
  scan     --focal focal rows at the middle of consecutive stretches of 2 x --extent rows, max_extent = --extent, no threshold, unit distance
  windows  the same stretches as windows of 2 x --extent rows
Both refine focal x 2 x extent rows (10^6 at the defaults).  Reported: kernel ms (the library's HIP events, best of --repeats after one
warm-up) and microseconds per refined row per compute unit = kernel time x CUs / rows refined, for both, and their ratio; the scan again
under every FMH_HAP_THREADS value, and a second case with fewer items than compute units (--few focal rows).
Before anything is timed the records of the focal rows inside the first --check-rows rows are compared with the numpy oracle
(tests/ehh_ref.py) on a second, small matrix generated with the same seed, and every record is checked for steps == max_extent.

Needs a GPU.  One JSON line per case to stdout and to profiles/ehh/measure_ehh.jsonl (or --out).
Default shape: 1 000 000 sites x 5 000 haplotypes; `tools/measure_ehh.py 200000x5000` for others."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ferromic_amd import _abi, device  # noqa: E402
from tests import ehh_ref  # noqa: E402
from tools.measure_haplotypes import device_cohort, thresholds, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--focal", type=int, default=2500)
    ap.add_argument("--few", type=int, default=64, help="focal rows of the case with fewer items than compute units")
    ap.add_argument("--extent", type=int, default=200)
    ap.add_argument("--cohorts", default="rare,monomorphic")
    ap.add_argument("--check-rows", type=int, default=2000)
    ap.add_argument("--threads", default="64,256,512,1024", help="FMH_HAP_THREADS values to time besides the default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ehh", "measure_ehh.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 5000)]
    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    import torch

    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:

        def emit(row):
            row["repeats"] = args.repeats  # best of this many timed calls after one warm-up
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for sites, n, kind in [(s, h, k) for s, h in shapes for k in args.cohorts.split(",") if k]:
            seed = sites + n
            thr = thresholds("rare", sites, seed) if kind == "rare" else np.zeros((1, sites), dtype=np.uint32)
            dm = device_cohort(thr, sites, n, seed)
            mask = np.ones(n, dtype=np.uint8)
            g = device.Groups(dm, mask[None, :])
            extent = args.extent
            params = _abi.EhhParams(0, 1, extent, 0, 0, 0)

            def focal_rows(count):
                count = min(count, sites // (2 * extent))
                return (extent + 2 * extent * np.arange(count)).astype(np.uint64)

            # ---- checks before timing
            check_rows = min(args.check_rows, sites)
            small = device_cohort(thr, check_rows, n, seed, keep_bytes=True)
            x = small.download()[0].reshape(check_rows, n)
            small.close()
            focal = focal_rows(args.focal)
            got = device.ehh_scan(dm, g, focal, max_extent=extent)
            inside = focal + np.uint64(extent) < check_rows
            ref = ehh_ref.scan(x, None, mask.astype(bool), focal[inside], max_extent=extent)[0]
            ok = all(np.array_equal(got.sides[inside][field], ref[field]) for field in ("area2", "pair_steps", "steps", "core", "flags"))
            walked = got.sides["steps"].max(axis=2)
            ok = ok and bool((walked[1:-1] == extent).all())
            emit({"case": f"{sites}x{n} {kind} check", "focal": int(len(focal)), "focal_checked_against_oracle": int(inside.sum()), "checks_pass": bool(ok),
                  "core1_min_median_max": [int(got.sides["core"][:, 0, 1].min()), float(np.median(got.sides["core"][:, 0, 1])), int(got.sides["core"][:, 0, 1].max())]})

            def scan_case(label, focal, threads):
                d_out = device.DeviceBuffer(dm.device, 56 * 2 * len(focal))
                call = lambda: _abi.check(lib.fmh_ehh_scan(dm._h, g._h, 0, sites, focal.ctypes.data_as(C.c_void_p), len(focal), None, C.byref(params),  # noqa: E731
                                                           d_out.ptr, None, None))
                with _abi.options(**({} if threads is None else {"FMH_HAP_THREADS": threads})):
                    kernel, wall = timed(call, args.repeats)
                sides = d_out.to_numpy(np.uint8, 56 * 2 * len(focal)).view(device.EHH_SIDE_DTYPE).reshape(len(focal), 2)
                d_out.free()
                rows = int(sides["steps"].max(axis=2).sum())
                row = {"case": f"{sites}x{n} {kind}: scan, {label}", "kernel": "fmh_ehh_scan", "sites": sites, "haplotypes": n, "focal": int(len(focal)),
                       "items": 2 * int(len(focal)), "max_extent": extent, "rows_refined": rows, "hap_threads": 0 if threads is None else threads,
                       "compute_units": cus, "checks_pass": bool(ok), "kernel_ms": kernel, "call_wall_ms": wall,
                       "us_per_refined_row_per_cu": kernel * 1e3 * cus / rows}
                emit(row)
                return row

            def window_case(label, focal, threads):
                w = np.stack([focal - np.uint64(extent), focal + np.uint64(extent)], axis=1)
                d_out = device.DeviceBuffer(dm.device, 24 * len(w))
                call = lambda: _abi.check(lib.fmh_haplotype_windows(dm._h, g._h, w.ctypes.data_as(C.c_void_p), len(w), d_out.ptr, None, None))  # noqa: E731
                with _abi.options(**({} if threads is None else {"FMH_HAP_THREADS": threads})):
                    kernel, wall = timed(call, args.repeats)
                d_out.free()
                rows = int((w[:, 1] - w[:, 0]).sum())
                row = {"case": f"{sites}x{n} {kind}: windows, {label}", "kernel": "fmh_haplotype_windows", "sites": sites, "haplotypes": n,
                       "windows": int(len(w)), "rows_refined": rows, "hap_threads": 0 if threads is None else threads, "compute_units": cus,
                       "kernel_ms": kernel, "call_wall_ms": wall, "us_per_refined_row_per_cu": kernel * 1e3 * cus / rows}
                emit(row)
                return row

            thread_values = [None] + [int(v) for v in args.threads.split(",") if v]
            for label, focal in ((f"{args.focal} focal x {extent}", focal_rows(args.focal)), (f"{args.few} focal x {extent}", focal_rows(args.few))):
                yard = window_case(label, focal, None)
                scans = [scan_case(label, focal, threads) for threads in thread_values]
                for threads in thread_values[1:]:
                    window_case(label, focal, threads)
                emit({"case": f"{sites}x{n} {kind}: ratio, {label}", "scan_us_per_row_per_cu": scans[0]["us_per_refined_row_per_cu"],
                      "windows_us_per_row_per_cu": yard["us_per_refined_row_per_cu"],
                      "ratio_scan_over_windows": scans[0]["us_per_refined_row_per_cu"] / yard["us_per_refined_row_per_cu"],
                      "best_scan_threads": min(scans[1:], key=lambda r: r["kernel_ms"])["hap_threads"] if len(scans) > 1 else 0})
            g.close()
            dm.close()


if __name__ == "__main__":
    main()
