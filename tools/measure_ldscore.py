#!/usr/bin/env python3
"""Development measurement of the LD scores' matrix-core kernel (fmh_ld_scores) against the popcount route that
counts the same pairs: fmh_clump with p1 = p2 = 1 (every site a candidate) over the same rows and window, in the same process.  Not a
test: no test asserts a time.

Per cohort (complete; about 1 % of the genotypes uncalled, which takes the MISSING core): the kernel time (HIP events inside the call,
fmh_timing_read; best of --repeats after a warm-up), the ordered pairs inside the windows, the pairs the 64 x 64 tiles compute, pairs per
second of both kernels and the int8 operations per second of the matrix-core kernel (2 x tile pairs x products x the samples the K loop
covers) as a share of the card's int8 dense peak (2.5 PMAC/s = 5 P op/s).  The window is given in participants
(sites; positions are row numbers).  Before timing, a 3 000-row slice of a second cohort of the same recipe is compared with
fmh_ld_scores_host.

Every cohort runs in a child process of its own under a time limit; a child that fails ends the run with its status, and when one runs out
of time nothing more is started.  One JSON line per case to stdout and to profiles/ldscore/measure_ldscore.jsonl (or --out).
Default shape: 200 000 sites x 5 000 haplotypes (2 500 samples); `tools/measure_ldscore.py 400000x5000` for others."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

INT8_PEAK_OPS_PER_S = 5.0e15   # 2.5 PMAC/s dense


def measure(sites, haplotypes, missing, repeats, windows, check_rows):
    from ferromic_amd import _abi, device
    from measure_ibd import dosages_of
    from measure_kinship import cohort
    from measure_sfs import timed

    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    n = haplotypes // 2
    label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")
    tile = device.LDSCORE_TILE
    products = 6 if missing else 1
    k_samples = -(-n // 128) * 128   # the K loop walks whole slabs of 128 samples

    # ---- check before timing: a second cohort of the same recipe against the host twin
    rows = min(sites, check_rows)
    small = cohort(rows, n, missing, seed=rows + n + 1)
    d = dosages_of(small, n)
    prm = device.ldscore_params(windows[0] // 2, True)
    got, twin = device.ld_scores(small, prm), device.ld_scores_host(d, prm)
    check = dict(checks_pass=bool(np.array_equal(got.q, twin.q) and np.array_equal(got.counted, twin.counted) and np.array_equal(got.partners, twin.partners)),
                 checked_rows=rows, checked_terms=int(twin.counted.sum()))
    small.close()
    del d

    dm = cohort(sites, n, missing, seed=sites + n)
    q, counted = np.zeros(sites, dtype=np.int64), np.zeros(sites, dtype=np.uint32)
    p, index_of = np.zeros(sites), np.zeros(sites, dtype=np.uint32)
    for window in windows:
        half = window // 2
        prm = device.ldscore_params(half, True)
        kernel, wall = timed(lambda: _abi.check(lib.fmh_ld_scores(dm._h, None, n, 0, sites, None, None, C.byref(prm), q.ctypes.data, None, counted.ctypes.data, None)),
                             repeats)
        rows_i = np.arange(sites)
        pairs = int((np.minimum(rows_i + half + 1, sites) - np.maximum(rows_i - half, 0)).sum())
        tiles = -(-sites // tile)
        last = np.minimum((np.arange(tiles) + 1) * tile, sites) - 1
        items = int(((np.minimum(last + half + 1, sites) - 1) // tile - np.arange(tiles) + 1).sum())
        diagonal = tiles
        tile_pairs = (2 * (items - diagonal) + diagonal) * tile * tile   # ordered pairs the tiles answer: an off-diagonal item serves both orders
        ops = 2 * items * tile * tile * products * k_samples
        cprm = device.clump_params(p1=1.0, p2=1.0, r2=0.5, window=half)
        clump_kernel, clump_wall = timed(lambda: _abi.check(lib.fmh_clump(dm._h, None, n, 0, sites, None, None, p.ctypes.data, C.byref(cprm), index_of.ctypes.data,
                                                                          None, None, None)), repeats)
        yield dict(check, case=f"{label}: fmh_ld_scores, window of {window} participants", sites=sites, haplotypes=haplotypes, samples=n, missing=missing,
                   core="MISSING" if missing else "complete", window_participants=window, repeats=repeats, kernel_ms=kernel, call_wall_ms=wall,
                   pairs_in_windows=pairs, items=items, tile_pairs=tile_pairs, products_per_pair=products, int8_ops=ops,
                   int8_ops_per_s=ops / (kernel * 1e-3) if kernel else None, share_of_int8_peak=ops / (kernel * 1e-3) / INT8_PEAK_OPS_PER_S if kernel else None,
                   window_pairs_per_s=pairs / (kernel * 1e-3) if kernel else None, clump_kernel_ms=clump_kernel, clump_wall_ms=clump_wall,
                   clump_window_pairs_per_s=pairs / (clump_kernel * 1e-3) if clump_kernel else None,
                   clump_kernel_over_ldscore_kernel=clump_kernel / kernel if kernel and clump_kernel else None)
    dm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--windows", default="200,1000", help="comma-separated window widths in participants")
    ap.add_argument("--check-rows", type=int, default=3000)
    ap.add_argument("--step-seconds", type=int, default=300, help="time limit of one cohort's child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldscore", "measure_ldscore.jsonl"))
    ap.add_argument("--child", nargs=3, metavar=("SITES", "HAPLOTYPES", "MISSING"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    windows = [int(v) for v in args.windows.split(",")]
    if args.child:
        for r in measure(int(args.child[0]), int(args.child[1]), args.child[2] == "1", args.repeats, windows, args.check_rows):
            print(json.dumps(r), flush=True)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(200_000, 5000)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for sites, haplotypes in shapes:
            for missing in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--windows", args.windows, "--check-rows", str(args.check_rows),
                       "--child", str(sites), str(haplotypes), "1" if missing else "0"]
                try:
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
                except subprocess.TimeoutExpired:
                    print(f"measure_ldscore: {sites}x{haplotypes} missing={missing} ran out of its {args.step_seconds} s: stopping", file=sys.stderr)
                    return 124
                lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
                for ln in lines:
                    print(ln, flush=True)
                    out.write(ln + "\n")
                out.flush()
                if res.returncode != 0:
                    print(res.stderr[-3000:], file=sys.stderr)
                    print(f"measure_ldscore: the child of {sites}x{haplotypes} missing={missing} ended with status {res.returncode}: stopping", file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
