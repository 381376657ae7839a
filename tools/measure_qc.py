#!/usr/bin/env python3
"""Development measurement of the genotype QC kernels (fmh_genotype_counts, fmh_hwe_exact) beside the two sweeps that read the same planes
of the same matrix in the same process: fmh_fstat_moments at G = 2 and the two-group fmh_population_summaries sweep with its per-site
tracks (DESIGN.md section 3.15's figures, measured again here).  Nothing about the QC kernels was measured before, so no ratio is fixed in
advance.

Cohort: fmh_matrix_generate, diploid, biallelic, allele frequencies skewed to rare alleles, packed; once complete and once with about 1 % of
the genotypes uncalled (tools/measure_kinship.py's cohorts).

Per cohort, the library's HIP-event kernel time (fmh_timing_read) and the wall time of the whole call, best of --repeats after one warm-up,
of: site tracks only; sample tables only; both; the weighted pass (weights from the tracks, fmh_genotype_site_weights); the exact test on the
resulting tracks; the two yardsticks.  Each with the bytes of the planes it reads (plane 0, and the called plane where a row has an uncalled
column; the weighted pass reads the called plane alone and nothing of a complete matrix) as TB/s at the kernel time.  Before anything is
timed the sample tables are checked against an algebra that shares nothing with them: the diagonals of fmh_kinship_counts' Grams over the
first --check-rows rows, and the tracks against the tables' totals.

Needs a GPU.  One JSON line per case to stdout and to profiles/qc/measure_qc.jsonl (or --out).
Default shape: 10 000 000 sites x 5 000 haplotypes; `tools/measure_qc.py 1000000x5000` for others."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ferromic_amd import _abi, device  # noqa: E402
from measure_kinship import cohort  # noqa: E402
from measure_sfs import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc", "measure_qc.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(10_000_000, 5000)]
    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile

        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for sites, haplotypes in shapes:
            n = haplotypes // 2
            plane_bytes = sites * ((haplotypes + 127) // 128 * 16)
            for missing in (False, True):
                dm = cohort(sites, n, missing, seed=sites + n)
                label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")

                # ---- checks before timing
                check_rows = min(sites, args.check_rows)
                kin = device.kinship_counts(dm, row_count=check_rows)
                part = device.genotype_counts(dm, row_count=check_rows)
                called = part.sample["hom_ref"] + part.sample["het"] + part.sample["hom_alt"]
                ok = (np.array_equal(kin.both.diagonal(), called) and np.array_equal(kin.het_het.diagonal(), part.sample["het"])
                      and all(int(part.site[k].sum(dtype=np.uint64)) == int(part.sample[k].sum()) for k in device.QC_CLASSES)
                      and (missing or bool((called == check_rows).all())))
                del kin, part

                tracks = [device.DeviceBuffer(dm.device, 4 * sites) for _ in range(3)]
                tables = device.GenotypeSampleBuffers(dm.device, n, device.QC_CLASSES + ("weighted_called",))
                site = _abi.GenotypeSiteOut(*[t.ptr for t in tracks])
                counted = _abi.GenotypeSampleOut(*[tables.bufs[k].ptr for k in device.QC_CLASSES], None)
                weighted = _abi.GenotypeSampleOut(None, None, None, tables.bufs["weighted_called"].ptr)
                d_p = device.DeviceBuffer(dm.device, 8 * sites)

                def counts(site_out, sample_out, weights=None):
                    return lambda: _abi.check(lib.fmh_genotype_counts(dm._h, None, n, 0, sites, None, None if weights is None else weights.ctypes.data_as(C.c_void_p),
                                                                      None if site_out is None else C.byref(site_out),
                                                                      None if sample_out is None else C.byref(sample_out), None, None))

                def case(what, call, read_bytes):
                    kernel, wall = timed(call, args.repeats)
                    emit({"case": f"{label}: {what}", "sites": sites, "haplotypes": haplotypes, "missing": missing, "checks_pass": bool(ok),
                          "item_rows": _abi.get_option("FMH_QC_ITEM_ROWS") or device.QC_DEFAULT_ITEM_ROWS, "kernel_ms": kernel, "call_wall_ms": wall,
                          "bytes_read": read_bytes, "tb_per_s_at_kernel_ms": read_bytes / (kernel * 1e-3) / 1e12 if kernel and read_bytes else None})
                    return kernel

                read = plane_bytes * (2 if missing else 1)
                case("site tracks only", counts(site, None), read)
                case("sample tables only", counts(None, counted), read)
                case("site tracks and sample tables", counts(site, counted), read)
                host = [t.to_numpy(np.uint32, sites) for t in tracks]
                weights = device.genotype_site_weights(*host)
                case("weighted pass", counts(None, weighted, weights), plane_bytes if missing else 0)
                case("HWE exact test on the tracks", lambda: _abi.check(lib.fmh_hwe_exact(site.d_hom_ref, site.d_het, site.d_hom_alt, sites, d_p.ptr, dm.device, None)),
                     sites * 20)
                del host, weights
                for t in tracks + [d_p]:
                    t.free()

                # ---- the yardsticks: two groups (the two halves of the columns) through the moment kernel and the summaries sweep
                masks = np.zeros((2, haplotypes), dtype=np.uint8)
                masks[0, : haplotypes // 2] = 1
                masks[1, haplotypes // 2:] = 1
                blocks = np.array([[0, sites]], dtype=np.uint64)
                table = device.DeviceBuffer(dm.device, 8 * device.fstat_moment_count(2))
                case("yardstick fmh_fstat_moments, G = 2",
                     lambda: _abi.check(lib.fmh_fstat_moments(dm._h, masks.ctypes.data_as(C.c_void_p), 2, blocks.ctypes.data_as(C.c_void_p), 1, table.ptr, None, None)),
                     read)
                table.free()
                g = device.Groups(dm, masks)
                yard = [device.DeviceBuffer(dm.device, 4 * 2 * sites) for _ in range(2)]
                totals = (_abi.PopTotals * 2)()
                case("yardstick fmh_population_summaries, two groups, per-site tracks",
                     lambda: _abi.check(lib.fmh_population_summaries(dm._h, g._h, 0, sites, device.FORMULA_SUMMARY, yard[0].ptr, yard[1].ptr, totals, None)), read)
                for t in yard:
                    t.free()
                g.close()
                dm.close()


if __name__ == "__main__":
    main()
