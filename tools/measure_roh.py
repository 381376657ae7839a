#!/usr/bin/env python3
"""Development measurement of the runs-of-homozygosity scan (fmh_roh_scan) beside two yardsticks on the same matrix in the same process:
(a) the time to read the planes the scan reads ONCE at the bandwidth a sweep reaches on them (fmh_population_summaries over every other
column, no site tracks; its kernel time and the bytes of the planes give the bandwidth), and (b) the host twin fmh_roh_scan_host on the host's
cores.  No speed figure is fixed in advance; DESIGN.md section 3.21 records what this prints and whether the kernel is bound by the
per-lane integer walk, as its code suggests, or by memory.

Cohort: fmh_matrix_generate, diploid, biallelic, allele frequencies skewed to rare alleles, packed; once complete and once with about 1 % of
the genotypes uncalled (tools/measure_kinship.py's cohorts).  PLINK's window (W = 50, one het, five missing calls, threshold 0.05); the
filters are loosened to the cohort (row numbers as positions), since the kernel's work does not depend on them.

Per cohort, the library's HIP-event kernel time (fmh_timing_read: flags, scan and stitch kernels) and the wall time of the whole call, best
of --repeats after one warm-up, tables only and with a segment buffer; the (row, sample) steps per second; the ratio to (a).  The host twin
runs over a second cohort of the same recipe with --host-rows rows (downloaded to build its state table), the samples split over
--host-threads threads (one call each, on a contiguous copy of its columns), and is scaled to all rows by the row ratio: its time is
linear in the rows.  Before anything is timed the device's tables over that cohort are compared with the twin's.

Needs a GPU.  Every cohort is measured by a child process of its own under a time limit (--step-seconds); after a child that fails or runs
out of time nothing more is started.  One JSON line per case to stdout and to profiles/roh/measure_roh.jsonl (or --out).
Default shape: 1 000 000 sites x 5 000 haplotypes (2 500 samples); `tools/measure_roh.py 2000000x5000` for others."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def states_of(dm):
    """[variants][n] uint8 states (0 HOM, 1 HET, 2 MISS) of a matrix, from its download."""
    data, words = dm.download()
    x = data.reshape(dm.variants, dm.columns)
    a, b = x[:, 0::2], x[:, 1::2]
    ok = (a <= 1) & (b <= 1)
    if words is not None:
        miss = np.unpackbits(words.view(np.uint8), bitorder="little")[: x.size].reshape(x.shape).astype(bool)
        ok &= ~(miss[:, 0::2] | miss[:, 1::2])
    return np.where(ok, (a != b).astype(np.uint8), 2).astype(np.uint8)


def measure(sites, haplotypes, missing, repeats, host_rows, host_threads):
    """One cohort, in this process; yields one dict per case."""
    from ferromic_amd import _abi, device
    from measure_kinship import cohort
    from measure_sfs import timed

    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    n = haplotypes // 2
    plane_bytes = sites * ((haplotypes + 127) // 128 * 16)
    read = plane_bytes * (2 if missing else 1)
    dm = cohort(sites, n, missing, seed=sites + n)
    label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")
    params = device.roh_params(window=50, window_het=1, window_missing=5, threshold=0.05, min_sites=100, min_length=100, max_gap=0, max_bp_per_site=0)

    # ---- check before timing, and the host twin's time: a second cohort of the same recipe with host_rows rows
    rows = min(sites, host_rows)
    small = cohort(rows, n, missing, seed=rows + n + 1)
    st = states_of(small)
    got = device.roh_scan(small, params)
    small.close()
    chunks = [c for c in np.array_split(np.arange(n), host_threads) if c.size]
    copies = [np.ascontiguousarray(st[:, c]) for c in chunks]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=len(chunks)) as pool:   # ctypes releases the GIL around the call
        parts = list(pool.map(lambda s: device.roh_scan_host(s, params), copies))
    host_ms = (time.perf_counter() - t0) * 1e3
    ok = all(np.array_equal(np.concatenate([p.tables[name] for p in parts]), got.tables[name]) for name in device.ROH_TABLES)
    runs = int(got.tables["n_runs"].sum())
    del st, copies, parts, got

    # ---- (a) a sweep over the same planes: its bandwidth, and the planes of the scan once at that bandwidth
    # every other column: a group with members in every vector that is neither contiguous nor everyone, so the sweep has to read the rows
    # (the group of all columns is answered from the row totals and reads no plane)
    g = device.Groups(dm, (np.arange(haplotypes) % 2 == 0).astype(np.uint8)[None, :])
    totals = (_abi.PopTotals * 1)()
    sweep, _ = timed(lambda: _abi.check(lib.fmh_population_summaries(dm._h, g._h, 0, sites, _abi.FORMULA_SUMMARY, None, None, totals, None)), repeats)
    g.close()
    sweep_tb = read / (sweep * 1e-3) / 1e12 if sweep else None      # the sweep reads plane 0, and the called plane where there is one
    planes_once_ms = read / (sweep_tb * 1e12) * 1e3 if sweep_tb else None

    names = device.ROH_TABLES
    bufs = {name: device.DeviceBuffer(dm.device, 8 * n) for name in names}
    out = _abi.RohOut(*[bufs[name].ptr for name in names], None, None)
    seg = device.DeviceBuffer(dm.device, 64 * n * device.ROH_SEGMENT_DTYPE.itemsize)
    count = C.c_uint64(0)
    for what, call in (("tables only", lambda: lib.fmh_roh_scan(dm._h, None, n, 0, sites, None, None, C.byref(params), C.byref(out), None, 0, None, None)),
                       ("tables and segments", lambda: lib.fmh_roh_scan(dm._h, None, n, 0, sites, None, None, C.byref(params), C.byref(out), seg.ptr, 64 * n,
                                                                         C.byref(count), None))):
        kernel, wall = timed(lambda: _abi.check(call()), repeats)
        yield {"case": f"{label}: fmh_roh_scan, W = 50, {what}", "sites": sites, "haplotypes": haplotypes, "samples": n, "missing": missing,
               "checks_pass": ok, "runs_in_the_checked_rows": runs, "segments": int(count.value), "kernel_ms": kernel, "call_wall_ms": wall,
               "item_rows": _abi.get_option("FMH_ROH_ITEM_ROWS") or device.ROH_DEFAULT_ITEM_ROWS,
               "giga_row_sample_steps_per_s": sites * n / (kernel * 1e-3) / 1e9 if kernel else None,
               "plane_bytes_of_one_pass": read, "tb_per_s_at_kernel_ms": read / (kernel * 1e-3) / 1e12 if kernel else None,
               "sweep_kernel_ms": sweep, "sweep_tb_per_s": sweep_tb, "planes_once_at_sweep_bandwidth_ms": planes_once_ms,
               "kernel_ms_over_planes_once": kernel / planes_once_ms if kernel and planes_once_ms else None,
               "host_twin_rows": rows, "host_twin_threads": len(chunks), "host_twin_ms": host_ms, "host_twin_ms_scaled_to_all_rows": host_ms * sites / rows,
               "host_twin_scaled_over_kernel": host_ms * sites / rows / kernel if kernel else None}
    dm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of one cohort's child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roh", "measure_roh.jsonl"))
    ap.add_argument("--child", nargs=3, metavar=("SITES", "HAPLOTYPES", "MISSING"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        for r in measure(int(args.child[0]), int(args.child[1]), args.child[2] == "1", args.repeats, args.host_rows, args.host_threads):
            print(json.dumps(r), flush=True)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 5000)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for sites, haplotypes in shapes:
            for missing in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--host-rows", str(args.host_rows), "--host-threads",
                       str(args.host_threads), "--child", str(sites), str(haplotypes), "1" if missing else "0"]
                try:
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
                except subprocess.TimeoutExpired:
                    print(f"measure_roh: {sites}x{haplotypes} missing={missing} ran out of its {args.step_seconds} s: stopping", file=sys.stderr)
                    return 124
                lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
                for ln in lines:
                    print(ln, flush=True)
                    out.write(ln + "\n")
                out.flush()
                if res.returncode != 0:
                    print(res.stderr[-3000:], file=sys.stderr)
                    print(f"measure_roh: the child of {sites}x{haplotypes} missing={missing} ended with status {res.returncode}: stopping", file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
