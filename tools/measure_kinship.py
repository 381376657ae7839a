#!/usr/bin/env python3
"""Development measurement of fmh_kinship_counts beside fmh_pairwise_differences on the same matrix in the same
process: both run the same Gram kernels through the same launcher, so pairwise is the yardstick for the Gram and for the planes pass.

Cohorts: fmh_matrix_generate, biallelic, allele frequencies skewed to rare alleles, packed - one complete (the two-Gram route: H with the
all-ones row, and W) and one with about 1 % of the genotypes uncalled (0.5 % of the entries; the general route: [H; V] stacked, and W).

Per cohort, best of --repeats after one warm-up, by the library's HIP events (fmh_timing_read_gram): the planes kernel, each Gram (with its
slab reduce) and the finish kernel, and the same stages of fmh_pairwise_differences; the wall time of both calls; the same call with a sample list that is not the identity (the gathering staging); MACs (whole 256 x 256 tiles
of the upper triangle x kept sites), MAC/s of each Gram against the FP4 dense peak (5 PMAC/s) and against pairwise's Gram.  Before anything
is timed the tables are checked: symmetry and diagonals, and on the complete cohort the identity
diff = 2 het_het + 2 (het_hom + het_hom^T) + 4 ibs0 against fmh_pairwise_differences' table.

Needs a GPU.  One JSON line per cohort to stdout and to profiles/kinship/measure_kinship.jsonl (or --out), which the run REPLACES.
Default shape: 1 000 000 sites x 2 500 samples; `tools/measure_kinship.py 200000x500` for others."""
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

FP4_PEAK_MACS = 5.0e15  # dense FP4 MAC/s of an MI355X, as DESIGN.md section 3.7 counts it


def cohort(sites, samples, missing, seed):
    rng = np.random.default_rng(seed)
    freq = rng.beta(0.2, 2.0, size=sites)
    thr = (np.clip(freq, 0.0, 1.0) * float(1 << 24)).astype(np.uint32)[None, :]
    dm = device.DeviceMatrix.alloc(sites, samples, 2, missing, 1)
    dm.generate(seed, 0, thr, np.zeros(2 * samples, dtype=np.uint8), int(0.005 * (1 << 24)) if missing else 0)
    dm.pack(release_bytes=True)
    return dm


def tri(n_rows):
    nt = -(-n_rows // 256)
    return nt * (nt + 1) // 2


def staged(call, repeats):
    """(best stage ms [4], best wall ms) after one warm-up"""
    lib = _abi.load()
    best, best_wall = None, None
    for i in range(repeats + 1):
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 4)()
        _abi.check(lib.fmh_timing_read_gram(ms))
        if i and (best is None or sum(ms) < sum(best)):
            best = list(ms)
        if i:
            best_wall = wall if best_wall is None else min(best_wall, wall)
    return best, best_wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxSAMPLES")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinship", "measure_kinship.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 2500)]
    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for sites, n in shapes:
            for missing in (False, True):
                dm = cohort(sites, n, missing, seed=sites + n)
                got = device.kinship_counts(dm)
                diff, _ = device.pairwise_differences(dm, n)
                upper = np.triu(np.ones((n, n), dtype=bool), 1)
                ok = (np.array_equal(got.both, got.both.T) and np.array_equal(got.het_het, got.het_het.T) and np.array_equal(got.ibs0, got.ibs0.T)
                      and not got.ibs0.diagonal().any() and not got.het_hom.diagonal().any() and int(got.both.diagonal().max()) <= sites
                      and bool((got.both <= np.minimum.outer(got.both.diagonal(), got.both.diagonal())).all()))
                if not missing:
                    identity = 2 * got.het_het + 2 * (got.het_hom + got.het_hom.T) + 4 * got.ibs0
                    ok = ok and bool((got.both == sites).all()) and np.array_equal(identity[upper], diff[upper])
                del got, diff

                bufs = device.KinshipBuffers(dm.device, n)
                kin_ms, kin_wall = staged(lambda: _abi.check(lib.fmh_kinship_counts(dm._h, None, n, 0, sites, None, C.byref(bufs.out), None, None)),
                                          args.repeats)
                d_diff, d_both = device.DeviceBuffer(dm.device, 8 * n * n), device.DeviceBuffer(dm.device, 8 * n * n)
                pd_ms, pd_wall = staged(lambda: _abi.check(lib.fmh_pairwise_differences(dm._h, n, d_diff.ptr, d_both.ptr, None)), args.repeats)

                rows_a = (2 * n if missing else n) + 1
                macs_a, macs_w = tri(rows_a) * 65536 * sites, tri(n) * 65536 * sites
                pd_planes = 4 if missing else 1  # two allele planes, length and valid with missing calls; else one plane and the all-ones row
                macs_pd = pd_planes * tri(n + (0 if missing else 1)) * 65536 * sites
                row = {"case": f"{sites}x{n} {'about 1 % of the genotypes uncalled (general route)' if missing else 'complete (two n-row Grams)'}",
                       "sites": sites, "samples": n, "missing": missing, "checks_pass": bool(ok),
                       "operands": "int8" if _abi.get_option("FMH_PD_INT8") else "fp4",
                       "kin_planes_ms": kin_ms[0], "kin_gram_a_ms": kin_ms[1], "kin_gram_w_ms": kin_ms[2], "kin_finish_ms": kin_ms[3],
                       "kin_kernels_ms": sum(kin_ms), "kin_call_wall_ms": kin_wall,
                       "kin_gram_a_macs": macs_a, "kin_gram_w_macs": macs_w,
                       "kin_gram_a_pmac_per_s": macs_a / (kin_ms[1] * 1e-3) / 1e15, "kin_gram_w_pmac_per_s": macs_w / (kin_ms[2] * 1e-3) / 1e15,
                       "kin_grams_of_fp4_peak": (macs_a + macs_w) / ((kin_ms[1] + kin_ms[2]) * 1e-3) / FP4_PEAK_MACS,
                       "pairwise_planes_ms": pd_ms[0], "pairwise_grams_ms": pd_ms[1], "pairwise_finish_ms": pd_ms[3], "pairwise_kernels_ms": sum(pd_ms),
                       "pairwise_call_wall_ms": pd_wall, "pairwise_macs": macs_pd, "pairwise_pmac_per_s": macs_pd / (pd_ms[1] * 1e-3) / 1e15,
                       "kin_grams_mac_rate_over_pairwise": ((macs_a + macs_w) / (kin_ms[1] + kin_ms[2])) / (macs_pd / pd_ms[1]),
                       "kin_planes_over_pairwise_planes": kin_ms[0] / pd_ms[0]}
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                # the gathering staging of the planes kernel: a sample list that is not 0 .. n-1 (every sample but the first)
                some = np.arange(1, n, dtype=np.uint32)
                part = device.KinshipBuffers(dm.device, n - 1)
                list_ms, list_wall = staged(lambda: _abi.check(lib.fmh_kinship_counts(dm._h, some.ctypes.data_as(C.c_void_p), n - 1, 0, sites, None,
                                                                                       C.byref(part.out), None, None)), args.repeats)
                line = json.dumps({"case": row["case"] + ", sample list 1 .. n-1 (gathering staging)", "sites": sites, "samples": n - 1, "missing": missing,
                                   "operands": row["operands"], "kin_planes_ms": list_ms[0], "kin_gram_a_ms": list_ms[1], "kin_gram_w_ms": list_ms[2],
                                   "kin_finish_ms": list_ms[3], "kin_kernels_ms": sum(list_ms), "kin_call_wall_ms": list_wall,
                                   "kin_planes_over_identity_planes": list_ms[0] / kin_ms[0]})
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                dm.close()


if __name__ == "__main__":
    main()
