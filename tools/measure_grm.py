#!/usr/bin/env python3
"""Development measurement of the genomic relationship matrix (fmh_grm, fmh_grm_eigen): per shape the stage times - the codes kernel, the
Gram with its split-K reduce and the addition into the caller's matrix (HIP events inside the library, fmh_timing_read_grm), the host
finish, the eigen solver (fmh_timing_read_pca's event time of rocsolver_dsyevd) - best of --repeats after a warm-up, the Gram's f64
TFLOP/s counting the n (n + 1) / 2 * m * 2 flops of the upper triangle against the 78.6 TFLOP/s matrix peak, and in the same process two
baselines of the Gram stage: (a) fmh_pca_gram over the same rows of the cohort's 2 n haplotypes (complete cohorts only) - the route this
kernel replaces, four times the flops - and (b) torch.mm(Z, Z.T) in f64 on a materialised Z (torch is only this tool's yardstick, never a
dependency of the library).  A 64-sample corner of S is checked against tests/grm_ref.py.

Needs a GPU.  One JSON line per case to stdout and to profiles/grm/measure_grm.jsonl (or the path given with --out).
Cases: SAMPLESxROWS[m] (m = about 1 % of the genotypes missing), default 2500x200000 2500x200000m 1000x150000."""
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
from tests import grm_ref as R  # noqa: E402

PEAK_F64_MATRIX_TFLOPS = 78.6


def read(fn, count):
    ms = (C.c_double * count)()
    _abi.check(fn(ms))
    return list(ms)


def torch_mm_ms(n, m, repeats):
    import torch

    z = torch.randn(n, m, dtype=torch.float64, device="cuda")
    torch.mm(z, z.T)
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.mm(z, z.T)
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b)
        best = t if best is None else min(best, t)
    del z
    torch.cuda.empty_cache()
    return best


def device_cohort(samples, rows, seed, missing, populations=5, scale=0.08):
    """A five-population cohort written by the library's counter-based generator straight into device memory, packed to bit planes;
    returns (matrix, the first 128 columns of its host copy, their called flags or None)."""
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=rows)
    thr = np.stack([np.clip(base + rng.normal(0.0, scale, size=rows), 0.001, 0.999) for _ in range(populations)])
    n = 2 * samples
    dm = device.DeviceMatrix.alloc(rows, samples, 2, missing, 1)
    dm.generate(seed, 0, (thr * float(1 << 24)).astype(np.uint32), (np.arange(n) * populations // n).astype(np.uint8), int(0.005 * (1 << 24)) if missing else 0)
    data, words = dm.download()
    corner = np.ascontiguousarray(data.reshape(rows, n)[:, :128])
    called = None
    if words is not None:
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[: rows * n].reshape(rows, n)
        called = np.ascontiguousarray(bits[:, :128] == 0)
    del data, words
    dm.pack(release_bytes=True)
    return dm, corner, called


def measure(samples, rows, missing, repeats, with_torch):
    lib = _abi.load()
    dm, corner, called = device_cohort(samples, rows, samples + rows, missing)
    site = device.genotype_counts(dm, sample=None).site
    c = site["hom_ref"].astype(np.int64) + site["het"] + site["hom_alt"]
    a = site["het"].astype(np.int64) + 2 * site["hom_alt"]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = a / (2.0 * c)
    keep = (c > 0) & (np.minimum(p, 1.0 - p) >= 0.05)  # the caller's filter: MAF >= 5 %
    best = None
    for i in range(repeats + 1):
        got = device.grm(dm, keep=keep)
        ms = read(lib.fmh_timing_read_grm, 3)
        if i and (best is None or ms[1] + ms[2] < best[1] + best[2]):
            best = ms
    m = got.n_usable
    t0 = time.perf_counter()
    A = device.grm_finish(got.products, None, m, got.scale)
    finish_ms = (time.perf_counter() - t0) * 1e3
    solver_ms = None
    for _ in range(2):
        device.grm_eigen(dm.device, A, 10)
        pca = read(lib.fmh_timing_read_pca, 6)
        solver_ms, solver = pca[4], {1.0: "host", 2.0: "rocsolver"}[pca[5]]
    # a 64-sample corner against the oracle
    kept_rows = np.flatnonzero(keep)
    code = R.codes(corner[kept_rows], None if called is None else called[kept_rows])
    z = R.values(c[kept_rows].astype(np.uint32), a[kept_rows].astype(np.uint32))[2]
    Z = R.operands(code, z)
    err = np.abs(got.products[:64, :64] - Z @ Z.T)
    bound = R.bound(np.abs(Z) @ np.abs(Z).T, m + 64)
    flops = samples * (samples + 1) / 2 * m * 2
    gram_ms = best[1] + best[2]
    row = {"case": f"{samples}x{rows}{'m' if missing else ''}", "samples": samples, "rows": rows, "missing": missing, "usable_rows": m, "codes_ms": best[0],
           "gram_ms": best[1], "reduce_add_ms": best[2], "finish_ms": finish_ms, "eigen_solver_ms": solver_ms, "eigen_solver_that_ran": solver,
           "gram_f64_tflops": flops / (gram_ms * 1e-3) / 1e12, "gram_fraction_of_peak": flops / (gram_ms * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS,
           "corner_max_err_over_bound": float((err / bound).max())}
    if not missing:  # (a) the haplotype Gram over the same rows
        usable = kept_rows[got.usable].astype(np.uint64)
        ones = np.ones(usable.size)
        hap = None
        for i in range(repeats + 1):
            device.pca_gram_device(dm, usable, ones, -ones).free()
            ms = read(lib.fmh_timing_read_pca, 6)
            if i and (hap is None or ms[1] + ms[2] < hap):
                hap = ms[1] + ms[2]
        row["haplotype_gram_ms"] = hap
        row["gram_time_over_haplotype_gram"] = gram_ms / hap
    if with_torch and samples * m * 8 <= 24 << 30:  # (b)
        mm = torch_mm_ms(samples, m, repeats)
        row["torch_mm_f64_ms"] = mm
        row["torch_mm_f64_tflops"] = 2.0 * samples * samples * m / (mm * 1e-3) / 1e12
        row["gram_time_over_torch_mm"] = gram_ms / mm
    dm.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="SAMPLESxROWS, an m behind it for about 1 %% missing genotypes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grm", "measure_grm.jsonl"))
    args = ap.parse_args()
    cases = args.cases or ["2500x200000", "2500x200000m", "1000x150000"]
    _abi.check(_abi.load().fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for case in cases:
            missing = case.endswith("m")
            samples, rows = (int(v) for v in case.rstrip("m").split("x"))
            line = json.dumps(measure(samples, rows, missing, args.repeats, not args.no_torch))
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
