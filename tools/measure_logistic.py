#!/usr/bin/env python3
"""Development measurement of the logistic association scan's device side, each figure beside a yardstick taken in the same process on the
same matrix.  No speed figure is fixed in advance; DESIGN.md section 3.19 records what was measured.

  1. fmh_assoc_homalt_sums at K = 1, 4 and 16 value columns; yardstick: fmh_assoc_sums, S only, with the same columns over the same rows.
     It issues the same MFMAs with a cheaper operand, so level or ahead is the expectation (not a gate).  The kernel times include the
     digit preparation kernel on both sides.
  2. fmh_logistic_score for a batch of Pb = 8 phenotypes with c = 5 (K = 64); yardstick: the two device-to-host copies of S and C
     ([rows][64] i64 each) that the reduction on the device replaces, as wall time of fmh_copy_to_host into pageable host memory (what
     ferromic.association_scan does); beside it the copies of score and variance that remain.
  3. ferromic.Population.logistic_scan end to end (null models on the host, all chunks and batches, statistics) with c = 5 and P = 9, as wall
     time of the second call (the matrix is resident by then); yardstick: Population.association_scan with the same covariates and nine
     quantitative phenotypes.

Cohort of 1. and 2.: fmh_matrix_generate, diploid, biallelic, allele frequencies skewed to rare alleles, packed, once complete and once
with about 1 % of the genotypes uncalled (tools/measure_kinship.py's cohorts).  Before anything is timed H of a column of ones is checked
against the hom_alt track, and S - 2 H against the het track, over the first --check-rows rows, and the device scores against the host twin.

Needs a GPU.  Every part is measured by a child process of its own under a time limit (--step-seconds); after a child that fails or runs
out of time nothing more is started.  One JSON line per case to stdout and to profiles/logistic/measure_logistic.jsonl (or --out).
Default shape: 1 000 000 sites x 5 000 haplotypes (end to end: --scan-shape, default 100 000 x 2 000)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

COLUMNS = (1, 4, 16)


def measure_kernels(sites, haplotypes, missing, repeats, check_rows):
    """Parts 1 and 2 on one cohort, in this process; yields one dict per case."""
    from ferromic_amd import _abi, device
    from measure_kinship import cohort
    from measure_sfs import timed

    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    n = haplotypes // 2
    dm = cohort(sites, n, missing, seed=sites + n)
    label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    # ---- checks before timing: a column of ones against the tracks
    rows = min(sites, check_rows)
    ones = np.ones((n, 1), dtype=np.int32)
    H = device.assoc_homalt_sums(dm, ones, row_count=rows)
    S = device.assoc_sums(dm, ones, row_count=rows, called=False).dosage
    qc = device.genotype_counts(dm, row_count=rows, sample=())
    ok = bool(np.array_equal(H[:, 0], qc.site["hom_alt"].astype(np.int64)) and np.array_equal((S - 2 * H)[:, 0], qc.site["het"].astype(np.int64)))
    del H, S

    def row(what, kernel, wall, yardstick=None, **extra):
        return dict({"case": f"{label}: {what}", "sites": sites, "haplotypes": haplotypes, "missing": missing, "checks_pass": ok, "kernel_ms": kernel,
                     "call_wall_ms": wall, "ms_over_yardstick": (kernel if kernel else wall) / yardstick if yardstick else None}, **extra)

    # ---- 1. hom-alt sums beside the dosage sums
    rng = np.random.default_rng(sites)
    for k in COLUMNS:
        values = rng.integers(-(1 << 30), (1 << 30) + 1, size=(n, k), dtype=np.int64).astype(np.int32)
        d_out = device.DeviceBuffer(dm.device, 8 * sites * k)
        yard, wall = timed(lambda: _abi.check(lib.fmh_assoc_sums(dm._h, None, n, 0, sites, ptr(values), k, d_out.ptr, None, None)), repeats)
        yield row(f"yardstick fmh_assoc_sums, K = {k}, S only", yard, wall, columns=k)
        kernel, wall = timed(lambda: _abi.check(lib.fmh_assoc_homalt_sums(dm._h, None, n, 0, sites, ptr(values), k, d_out.ptr, None)), repeats)
        yield row(f"fmh_assoc_homalt_sums, K = {k}", kernel, wall, yard, columns=k,
                  item_rows=_abi.get_option("FMH_ASSOC_ITEM_ROWS") or device.ASSOC_DEFAULT_ITEM_ROWS)
        d_out.free()

    # ---- 2. the reduction on the device beside the copies it replaces: c = 5, Pb = 8, K = 64
    c, pb = 5, 8
    k = pb * (c + 3)
    y = (rng.random((n, pb)) < 0.3).astype(np.float64)
    model = device.logistic_null(y, rng.normal(size=(n, c)))
    values = model.values[0]
    wcol = np.ascontiguousarray(values[:, c + 2::c + 3])
    total, exponent = np.ascontiguousarray(model.total.reshape(-1)), np.ascontiguousarray(model.exponent.reshape(-1))
    d_s, d_c = device.DeviceBuffer(dm.device, 8 * sites * k), device.DeviceBuffer(dm.device, 8 * sites * k)
    d_h, d_u, d_v = [device.DeviceBuffer(dm.device, 8 * sites * pb) for _ in range(3)]
    tracks = [device.DeviceBuffer(dm.device, 4 * sites) for _ in range(3)]
    site = _abi.GenotypeSiteOut(*[t.ptr for t in tracks])
    _abi.check(lib.fmh_genotype_counts(dm._h, None, n, 0, sites, None, None, C.byref(site), None, None, None))
    _abi.check(lib.fmh_assoc_sums(dm._h, None, n, 0, sites, ptr(values), k, d_s.ptr, d_c.ptr, None))
    _abi.check(lib.fmh_assoc_homalt_sums(dm._h, None, n, 0, sites, ptr(wcol), pb, d_h.ptr, None))

    def score():
        _abi.check(lib.fmh_logistic_score(d_s.ptr, d_c.ptr, d_h.ptr, *[t.ptr for t in tracks], sites, ptr(total), ptr(exponent), c, pb, d_u.ptr, d_v.ptr,
                                          dm.device, None))

    score()
    part = min(sites, check_rows)
    host = device.logistic_score_host(d_s.to_numpy(np.int64, part * k), d_c.to_numpy(np.int64, part * k), d_h.to_numpy(np.int64, part * pb).reshape(part, pb),
                                      *[t.to_numpy(np.uint32, part) for t in tracks], total, exponent, c)
    got = [d.to_numpy(np.float64, part * pb).reshape(part, pb) for d in (d_u, d_v)]
    same = all(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))
               for a, b in zip(got, host))
    ok = ok and bool(same and model.fitted.all())

    big, small = np.empty(sites * k, dtype=np.int64), np.empty(sites * pb, dtype=np.float64)

    def copies(bufs, host_array):
        for b in bufs:
            _abi.check(lib.fmh_copy_to_host(dm.device, ptr(host_array), b.ptr, host_array.nbytes, None))

    _, yard = timed(lambda: copies((d_s, d_c), big), repeats)
    yield row(f"yardstick: device-to-host copies of S and C, [rows][{k}] i64 each", None, yard, bytes=2 * big.nbytes)
    kernel, wall = timed(score, repeats)
    yield row(f"fmh_logistic_score, c = {c}, Pb = {pb}", kernel, wall, yard, columns=k)
    _, wall = timed(lambda: copies((d_u, d_v), small), repeats)
    yield row(f"device-to-host copies of score and variance, [rows][{pb}] f64 each", None, wall, yard, bytes=2 * small.nbytes)
    dm.close()


def measure_scan(sites, haplotypes, repeats):
    """Part 3, in this process."""
    import ferromic as fm

    n = haplotypes // 2
    rng = np.random.default_rng(sites + n)
    geno = np.empty((sites, n, 2), dtype=np.int8)
    for at in range(0, sites, 10_000):   # in slabs: the random floats of the whole table would be eight times its size
        part = geno[at:at + 10_000]
        part[:] = rng.random(part.shape, dtype=np.float32) < rng.beta(0.5, 2.0, size=(part.shape[0], 1, 1))
        part[rng.random(part.shape[:2], dtype=np.float32) < 0.01] = -1
    pop = fm.Population.from_numpy("p", geno, np.arange(sites, dtype=np.int64), [(s, side) for s in range(n) for side in (0, 1)], sites)
    cov = rng.normal(size=(n, 5))
    y = (rng.random((n, 9)) < 0.3).astype(np.float64)
    q = rng.normal(size=(n, 9))

    def wall(call):
        best = None
        for i in range(repeats + 1):   # the first call uploads the matrix
            t0 = time.perf_counter()
            res = call()
            ms = (time.perf_counter() - t0) * 1e3
            if i:
                best = ms if best is None else min(best, ms)
        return best, res

    yard, _ = wall(lambda: pop.association_scan(q, cov))
    ms, scan = wall(lambda: pop.logistic_scan(y, cov))
    label = f"{sites}x{haplotypes} about 1 % of the genotypes uncalled, c = 5, P = 9"
    ok = bool(scan.fitted.all() and np.isfinite(scan.p).any())
    yield {"case": f"{label}: yardstick Population.association_scan", "sites": sites, "haplotypes": haplotypes, "checks_pass": ok, "call_wall_ms": yard}
    yield {"case": f"{label}: Population.logistic_scan", "sites": sites, "haplotypes": haplotypes, "checks_pass": ok, "call_wall_ms": ms,
           "ms_over_yardstick": ms / yard}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--scan-shape", default="100000x2000", help="SITESxHAPLOTYPES of the end-to-end scan")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=200_000)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of one child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logistic", "measure_logistic.jsonl"))
    ap.add_argument("--child", nargs=4, metavar=("PART", "SITES", "HAPLOTYPES", "MISSING"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        part, sites, haplotypes = args.child[0], int(args.child[1]), int(args.child[2])
        rows = measure_scan(sites, haplotypes, args.repeats) if part == "scan" else measure_kernels(sites, haplotypes, args.child[3] == "1", args.repeats,
                                                                                                    args.check_rows)
        for r in rows:
            print(json.dumps(r), flush=True)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 5000)]
    steps = [("kernels", s, h, m) for s, h in shapes for m in (False, True)]
    steps.append(("scan", *[int(v) for v in args.scan_shape.split("x")], True))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for part, sites, haplotypes, missing in steps:
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--check-rows", str(args.check_rows), "--child", part, str(sites),
                   str(haplotypes), "1" if missing else "0"]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
            except subprocess.TimeoutExpired:
                print(f"measure_logistic: {part} {sites}x{haplotypes} missing={missing} ran out of its {args.step_seconds} s: stopping", file=sys.stderr)
                return 124
            for ln in (ln for ln in res.stdout.splitlines() if ln.startswith("{")):
                print(ln, flush=True)
                out.write(ln + "\n")
            out.flush()
            if res.returncode != 0:
                print(res.stderr[-3000:], file=sys.stderr)
                print(f"measure_logistic: the child of {part} {sites}x{haplotypes} missing={missing} ended with status {res.returncode}: stopping", file=sys.stderr)
                return res.returncode if res.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
