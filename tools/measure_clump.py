#!/usr/bin/env python3
"""Development measurement of LD clumping's tile kernel (fmh_clump) against the paper VALU bound of DESIGN.md section 3.23 and against
fmh_ld_band over the same number of pairs in the same process.  No speed figure is fixed in advance and no test asserts a time.

Cohort: fmh_matrix_generate, diploid, biallelic, allele frequencies skewed to rare alleles, packed; once complete and once with about 1 % of
the genotypes uncalled (tools/measure_kinship.py's cohorts).  Every --every-th site is a candidate (p = 0), every site a participant
(p = 0.5 under p2 = 1), positions are row numbers and the window is half of --windows participants on either side.  The sites are
independent, so hardly anything is claimed: the kernel's work does not depend on the data.

Per cohort and window: the library's HIP-event kernel time (fmh_timing_read: the row-sum kernel of the complete core and the tile kernel,
every chunk; the r^2 of the members is not asked for) and the wall time of the call, best of --repeats after one warm-up.  `pairs_in_windows`
are the (candidate, participant) pairs the definition asks about, `tile_pairs` what the tiles compute; products x column bits per second
counts the tile pairs (2 products per pair in the complete core, 7 in the MISSING core, 2 x samples column bits) and stands beside the
bound of 2 VALU lane-operations per 32 column bits and product.  fmh_ld_band (r^2 asked for, haplotype rows) runs over candidates x window
pairs of the same matrix.  Before anything is timed the device's assignment over --check-rows rows of a second cohort of the same recipe
is compared with fmh_clump_host.

Needs a GPU.  Every cohort is measured by a child process of its own under a time limit (--step-seconds); after a child that fails or runs
out of time nothing more is started.  One JSON line per case to stdout and to profiles/clump/measure_clump.jsonl (or --out).
Default shape: 200 000 sites x 5 000 haplotypes (2 500 samples); `tools/measure_clump.py 400000x5000` for others."""
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

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9   # DESIGN.md section 3.11's figure
BOUND_PRODUCT_BITS_PER_S = VALU_LANE_OPS_PER_S * 32 / 2


def measure(sites, haplotypes, missing, repeats, every, windows, check_rows):
    from ferromic_amd import _abi, device
    from measure_ibd import dosages_of
    from measure_kinship import cohort
    from measure_sfs import timed

    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    n = haplotypes // 2
    label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")
    tile = 32 if missing else 64
    products = 7 if missing else 2

    def p_values(rows):
        p = np.full(rows, 0.5)
        p[::every] = 0.0
        return p

    # ---- check before timing: a second cohort of the same recipe against the host twin
    rows = min(sites, check_rows)
    small = cohort(rows, n, missing, seed=rows + n + 1)
    d = dosages_of(small, n)
    prm = device.clump_params(p1=0.01, p2=1.0, r2=0.01, window=windows[0] // 2)
    got = device.clump(small, p_values(rows), prm)
    twin = device.clump_host(d, p_values(rows), prm)
    check = dict(checks_pass=bool(np.array_equal(got.index_of, twin.index_of) and np.array_equal(got.r2.view(np.uint64), twin.r2.view(np.uint64))
                                  and got.n_clumps == twin.n_clumps),
                 checked_rows=rows, checked_clumps=got.n_clumps, checked_members=int((got.index_of != device.CLUMP_NONE).sum()) - got.n_clumps)
    small.close()
    del d

    dm = cohort(sites, n, missing, seed=sites + n)
    p = p_values(sites)
    index_of = np.zeros(sites, dtype=np.uint32)
    cand = np.arange(0, sites, every)
    for window in windows:
        half = window // 2
        prm = device.clump_params(p1=0.01, p2=1.0, r2=0.5, window=half)
        kernel, wall = timed(lambda: _abi.check(lib.fmh_clump(dm._h, None, n, 0, sites, None, None, p.ctypes.data, C.byref(prm), index_of.ctypes.data, None,
                                                              None, None)), repeats)
        lo, hi = np.maximum(cand - half, 0), np.minimum(cand + half + 1, sites)
        pairs = int((hi - lo).sum())
        items = 0
        for t in range(0, len(cand), tile):
            items += int((hi[min(t + tile, len(cand)) - 1] - 1) // 64 - lo[t] // 64 + 1)   # the windows of neighbouring candidates overlap: one run of tiles
        tile_pairs = items * tile * 64
        bits = tile_pairs * products * 2 * n
        band_kernel, band_wall = timed(lambda: device.ld_band(dm, None, window, row_count=len(cand), want=("r2",)), repeats)
        yield dict(check, case=f"{label}: fmh_clump, every {every}th site a candidate, window of {window} participants", sites=sites, haplotypes=haplotypes,
                   samples=n, missing=missing, core="MISSING" if missing else "complete", candidates=len(cand), window_participants=window, repeats=repeats,
                   kernel_ms=kernel, call_wall_ms=wall, pairs_in_windows=pairs, items=items, tile_pairs=tile_pairs, products_per_pair=products,
                   product_bits=bits, product_bits_per_s=bits / (kernel * 1e-3) if kernel else None,
                   paper_bound_product_bits_per_s=BOUND_PRODUCT_BITS_PER_S, share_of_bound=bits / (kernel * 1e-3) / BOUND_PRODUCT_BITS_PER_S if kernel else None,
                   ld_band_pairs=len(cand) * window, ld_band_kernel_ms=band_kernel, ld_band_wall_ms=band_wall,
                   clump_ns_per_window_pair=kernel * 1e6 / pairs if kernel else None, ld_band_ns_per_pair=band_kernel * 1e6 / (len(cand) * window) if band_kernel else None)
    dm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--every", type=int, default=20, help="every n-th site is a candidate")
    ap.add_argument("--windows", default="200,1000", help="comma-separated window widths in participants")
    ap.add_argument("--check-rows", type=int, default=3000)
    ap.add_argument("--step-seconds", type=int, default=300, help="time limit of one cohort's child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clump", "measure_clump.jsonl"))
    ap.add_argument("--child", nargs=3, metavar=("SITES", "HAPLOTYPES", "MISSING"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    windows = [int(v) for v in args.windows.split(",")]
    if args.child:
        for r in measure(int(args.child[0]), int(args.child[1]), args.child[2] == "1", args.repeats, args.every, windows, args.check_rows):
            print(json.dumps(r), flush=True)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(200_000, 5000)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for sites, haplotypes in shapes:
            for missing in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--every", str(args.every), "--windows", args.windows,
                       "--check-rows", str(args.check_rows), "--child", str(sites), str(haplotypes), "1" if missing else "0"]
                try:
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
                except subprocess.TimeoutExpired:
                    print(f"measure_clump: {sites}x{haplotypes} missing={missing} ran out of its {args.step_seconds} s: stopping", file=sys.stderr)
                    return 124
                lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
                for ln in lines:
                    print(ln, flush=True)
                    out.write(ln + "\n")
                out.flush()
                if res.returncode != 0:
                    print(res.stderr[-3000:], file=sys.stderr)
                    print(f"measure_clump: the child of {sites}x{haplotypes} missing={missing} ended with status {res.returncode}: stopping", file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
