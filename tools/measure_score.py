#!/usr/bin/env python3
"""Development measurement of the polygenic score's sums (fmh_score_sums) beside two yardsticks on the same planes of the same matrix in the
same process: fmh_genotype_counts with SAMPLE tables only (the existing one-pass per-sample reader) and fmh_assoc_sums at the same K (the
same contraction the other way).  No speed figure is fixed in advance; DESIGN.md section 3.20 records the measured ratios and on which side
of the plane traffic the kernel sits.

Cohort: fmh_matrix_generate, diploid, biallelic, allele frequencies skewed to rare alleles, packed; once complete and once with about 1 % of
the genotypes uncalled (tools/measure_kinship.py's cohorts).

Per cohort, the library's HIP-event kernel time (fmh_timing_read) and the wall time of the whole call, best of --repeats after one warm-up,
of fmh_score_sums at K = 1, 16 and 64 value columns, with and without the called sums C; each with the bytes of the planes a single pass
reads (plane 0, and the called plane of a cohort with uncalled genotypes) as TB/s at the kernel time, the useful int8 operations per second,
and the ratio to both yardsticks.  The kernel time of fmh_score_sums includes its digits and reduce kernels.  FMH_SCORE_BUDGET_BYTES is
raised to 4 GiB so that K = 64 with C runs as one call.  Before anything is timed the sums of a value column of ones are checked against
the QC sample tables over the first --check-rows rows (S = het + 2 hom_alt, C = the called count).

Needs a GPU.  Every cohort is measured by a child process of its own under a time limit (--step-seconds); after a child that fails or runs
out of time nothing more is started.  One JSON line per case to stdout and to profiles/score/measure_score.jsonl (or --out).
Default shape: 1 000 000 sites x 5 000 haplotypes; `tools/measure_score.py 2000000x5000` for others (at most 2^21 sites per call)."""
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

COLUMNS = (1, 16, 64)


def measure(sites, haplotypes, missing, repeats, check_rows):
    """One cohort, in this process; yields one dict per case."""
    from ferromic_amd import _abi, device
    from measure_kinship import cohort
    from measure_sfs import timed

    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    _abi.set_option("FMH_SCORE_BUDGET_BYTES", 4 << 30)
    n = haplotypes // 2
    plane_bytes = sites * ((haplotypes + 127) // 128 * 16)
    read = plane_bytes * (2 if missing else 1)
    dm = cohort(sites, n, missing, seed=sites + n)
    label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    # ---- checks before timing: a column of ones against the QC sample tables
    rows = min(sites, check_rows)
    ones = np.ones((rows, 1), dtype=np.int32)
    got = device.score_sums(dm, ones, ones, row_count=rows)
    qc = device.genotype_counts(dm, row_count=rows, site=())
    alt = qc.sample["het"].astype(np.int64) + 2 * qc.sample["hom_alt"].astype(np.int64)
    called = qc.sample["hom_ref"].astype(np.int64) + qc.sample["het"].astype(np.int64) + qc.sample["hom_alt"].astype(np.int64)
    ok = bool(np.array_equal(got.dosage[:, 0], alt) and np.array_equal(got.called[:, 0], called) and (missing or (called == rows).all()))
    del got, qc

    def row(what, kernel, wall, **extra):
        return dict({"case": f"{label}: {what}", "sites": sites, "haplotypes": haplotypes, "missing": missing, "checks_pass": ok, "kernel_ms": kernel,
                     "call_wall_ms": wall, "plane_bytes_of_one_pass": read, "tb_per_s_at_kernel_ms": read / (kernel * 1e-3) / 1e12 if kernel else None},
                    **extra)

    tables = device.GenotypeSampleBuffers(dm.device, n)
    yard, wall = timed(lambda: _abi.check(lib.fmh_genotype_counts(dm._h, None, n, 0, sites, None, None, None, C.byref(tables.out), None, None)), repeats)
    yield row("yardstick fmh_genotype_counts, sample tables only", yard, wall)

    rng = np.random.default_rng(sites)
    for k in COLUMNS:
        per_sample = rng.integers(-(1 << 30), (1 << 30) + 1, size=(n, k), dtype=np.int64).astype(np.int32)
        V = rng.integers(-(1 << 30), (1 << 30) + 1, size=(sites, k), dtype=np.int64).astype(np.int32)
        U = rng.integers(-(1 << 30), (1 << 30) + 1, size=(sites, k), dtype=np.int64).astype(np.int32)
        a_s, a_c = device.DeviceBuffer(dm.device, 8 * sites * k), device.DeviceBuffer(dm.device, 8 * sites * k)
        d_s, d_c = device.DeviceBuffer(dm.device, 8 * n * k), device.DeviceBuffer(dm.device, 8 * n * k)
        for with_called in (False, True):
            assoc, _ = timed(lambda: _abi.check(lib.fmh_assoc_sums(dm._h, None, n, 0, sites, p(per_sample), k, a_s.ptr,
                                                                  a_c.ptr if with_called else None, None)), repeats)
            kernel, wall = timed(lambda: _abi.check(lib.fmh_score_sums(dm._h, None, n, 0, sites, p(V), p(U) if with_called else None, k, d_s.ptr,
                                                                      d_c.ptr if with_called else None, None)), repeats)
            contractions = 2 if with_called and missing else 1
            yield row(f"fmh_score_sums, K = {k}, " + ("S and C" if with_called else "S only"), kernel, wall, columns=k, called_sums=with_called,
                      item_rows=_abi.get_option("FMH_SCORE_ITEM_ROWS") or device.SCORE_DEFAULT_ITEM_ROWS,
                      int8_tera_ops_per_s=2.0 * sites * n * 4 * k * contractions / (kernel * 1e-3) / 1e12 if kernel else None,
                      genotype_counts_kernel_ms=yard, kernel_ms_over_genotype_counts=kernel / yard if kernel and yard else None,
                      assoc_sums_kernel_ms=assoc, kernel_ms_over_assoc_sums=kernel / assoc if kernel and assoc else None)
        for b in (a_s, a_c, d_s, d_c):
            b.free()
    dm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=200_000)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of one cohort's child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score", "measure_score.jsonl"))
    ap.add_argument("--child", nargs=3, metavar=("SITES", "HAPLOTYPES", "MISSING"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        for r in measure(int(args.child[0]), int(args.child[1]), args.child[2] == "1", args.repeats, args.check_rows):
            print(json.dumps(r), flush=True)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 5000)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for sites, haplotypes in shapes:
            for missing in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--check-rows", str(args.check_rows), "--child", str(sites),
                       str(haplotypes), "1" if missing else "0"]
                try:
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
                except subprocess.TimeoutExpired:
                    print(f"measure_score: {sites}x{haplotypes} missing={missing} ran out of its {args.step_seconds} s: stopping", file=sys.stderr)
                    return 124
                lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
                for ln in lines:
                    print(ln, flush=True)
                    out.write(ln + "\n")
                out.flush()
                if res.returncode != 0:
                    print(res.stderr[-3000:], file=sys.stderr)
                    print(f"measure_score: the child of {sites}x{haplotypes} missing={missing} ended with status {res.returncode}: stopping", file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
