#!/usr/bin/env python3
"""Development measurement of the haplotype PCA (fmh_pca_*): per shape the stage times - site scan, gather + transpose, Gram,
split-K reduce, the eigen solver (HIP events inside the library, fmh_timing_read_pca; the whole eigen + scores call with its copies also
by the host clock) - the
Gram's f64 TFLOP/s counting the n (n + 1) / 2 * m * 2 flops of the upper triangle, torch.mm(Z, Z.T) in f64 on the same device where a
materialised Z fits (torch is only this tool's yardstick, never a dependency of the library), the largest Gram error against its
bound on a corner and on 2 000 random entries, and on the reference's four benchmark shapes the score error against 32 * d0 (tests/test_gpu_pca.py has the rule).

Needs a GPU.  One JSON line per shape to stdout and to profiles/pca/measure_pca.jsonl (or the path given with --out).
Shapes: haplotypes x sites, e.g. `tools/measure_pca.py 2000x150000 5000x200000`; default: those two and the four benchmark cohorts."""
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
from tests import pca_ref as R  # noqa: E402

PYBENCH = [(512, 48), (4096, 96), (16384, 128), (65536, 256)]  # variants x samples
EPS = 2.0 ** -53


def stage_times(dm, kept, hi, lo, repeats):
    """Best-of-`repeats` event times (ms) of the three kernels of fmh_pca_gram, after one warm-up call."""
    best = None
    buf = None
    for i in range(repeats + 1):
        buf = device.pca_gram_device(dm, kept, hi, lo)
        ms = stages()
        if i and (best is None or ms[1] < best[1]):
            best = ms[:3]
    return best, buf


def stages():
    ms = (C.c_double * 6)()
    _abi.check(_abi.load().fmh_timing_read_pca(ms))
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


def device_cohort(n, sites, seed, populations=5, scale=0.08):
    """A five-population cohort written by the library's counter-based generator straight into device memory (no host matrix of
    10^9 entries), packed to bit planes; returns (matrix, its host copy as (sites, n) uint8)."""
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=sites)
    thr = np.stack([np.clip(base + rng.normal(0.0, scale, size=sites), 0.001, 0.999) for _ in range(populations)])
    dm = device.DeviceMatrix.alloc(sites, n // 2, 2, False, 1)
    dm.generate(seed, 0, (thr * float(1 << 24)).astype(np.uint32), (np.arange(n) * populations // n).astype(np.uint8))
    flat = dm.download()[0].reshape(sites, n)
    dm.pack(release_bytes=True)
    return dm, flat


def measure(dm, flat, n, label, repeats, with_torch, scores_of=None):
    """dm: the device matrix; flat: its (variants, n) uint8 0/1 host copy."""
    variants = flat.shape[0]
    device.pca_scan_sites(dm)
    scan_ms = None
    for _ in range(repeats):
        alt, flags = device.pca_scan_sites(dm)
        scan_ms = stages()[3] if scan_ms is None else min(scan_ms, stages()[3])
    freq = alt.astype(np.float64) / float(n)
    kept = np.nonzero((flags == 0) & (np.minimum(freq, 1.0 - freq) >= 0.05))[0].astype(np.uint64)
    m = int(kept.size)
    hi, lo = R.set_clear_values(alt[kept.astype(np.int64)], n)
    (transpose_ms, gram_ms, reduce_ms), buf = stage_times(dm, kept, hi, lo, repeats)
    got = buf.to_numpy(np.float64, n * n).reshape(n, n)
    c = min(n, 128)
    z = np.where(flat[kept.astype(np.int64)][:, :c].T == 1, hi[None, :], lo[None, :])
    err = np.abs(got[:c, :c] - z @ z.T / float(n - 1))
    bound = 2.0 * (m + 2) * EPS * (np.abs(z) @ np.abs(z).T) / float(n - 1)
    # 2 000 random entries besides the corner
    rng = np.random.default_rng(n + m)
    ii, jj = rng.integers(n, size=2000), rng.integers(n, size=2000)
    worst_random = 0.0
    xk = flat[kept.astype(np.int64)]
    for lo_i in range(0, 2000, 100):
        sel = slice(lo_i, lo_i + 100)
        zi = np.where(xk[:, ii[sel]].T == 1, hi[None, :], lo[None, :])
        zj = np.where(xk[:, jj[sel]].T == 1, hi[None, :], lo[None, :])
        exact = (zi * zj).sum(axis=1) / float(n - 1)
        b = 2.0 * (m + 2) * EPS * (np.abs(zi) * np.abs(zj)).sum(axis=1) / float(n - 1)
        worst_random = max(worst_random, float((np.abs(got[ii[sel], jj[sel]] - exact) / b).max()))
    k = min(6, n)
    device.pca_eigen_scores(dm.device, got, k)
    t0 = time.perf_counter()
    device.pca_eigen_scores(dm.device, got, k)
    eigen_ms = (time.perf_counter() - t0) * 1e3  # the whole call: upload of the Gram, solver, download of the top vectors
    solver_ms, solver = stages()[4], {1.0: "host", 2.0: "rocsolver"}[stages()[5]]
    flops = n * (n + 1) / 2 * m * 2
    row = {"case": label, "haplotypes": n, "sites": variants, "kept_sites": m, "scan_ms": scan_ms, "transpose_ms": transpose_ms, "gram_ms": gram_ms,
           "reduce_ms": reduce_ms, "eigen_solver_ms": solver_ms, "eigen_scores_call_ms": eigen_ms, "gram_f64_tflops": flops / ((gram_ms + reduce_ms) * 1e-3) / 1e12,
           "gram_corner_max_err": float(err.max()), "gram_corner_max_err_over_bound": float((err / bound).max()),
           "gram_random_entries_max_err_over_bound": worst_random, "eigen_solver_that_ran": solver}
    if with_torch and n * m * 8 <= 24 << 30:
        mm = torch_mm_ms(n, m, repeats)
        row["torch_mm_f64_ms"] = mm
        row["torch_mm_f64_tflops"] = 2.0 * n * n * m / (mm * 1e-3) / 1e12
        row["gram_time_over_torch_mm"] = (gram_ms + reduce_ms) / mm
    if scores_of is not None:
        import ferromic as fm

        g = scores_of
        kept_ref, complete = R.site_filter(g)
        x = R.haplotype_matrix(g, kept_ref)
        kk = R.clamp_components(6, complete, n)
        a, _ = R.transform(x, kk)
        a = R.canonical_signs(a)
        d0 = float(np.abs(a - R.canonical_signs(R.transform_svd(x, kk))).max())
        res = fm.chromosome_pca({"genotypes": g, "positions": np.arange(g.shape[0], dtype=np.int64)}, [f"s{i}" for i in range(g.shape[1])], 6)
        serr = float(np.abs(R.canonical_signs(res.coordinates) - a).max())
        row.update({"score_max_err": serr, "score_32_d0": 32 * d0, "score_within_1.28e-10": bool(serr <= 1.28e-10)})
    dm.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="HAPLOTYPESxSITES")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-pybench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca", "measure_pca.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(2000, 150_000), (5000, 200_000)]
    _abi.check(_abi.load().fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for n, sites in shapes:
            dm, flat = device_cohort(n, sites, seed=n + sites)
            emit(measure(dm, flat, n, f"five populations {n}x{sites}", args.repeats, not args.no_torch))
        if not args.no_pybench:
            for variants, samples in PYBENCH:
                g = R.pybench_cohort(variants, samples, seed=variants + samples)
                flat = g.reshape(variants, 2 * samples).astype(np.uint8)
                dm = device.DeviceMatrix.from_host(flat, None, variants, samples, 2, 1)
                emit(measure(dm, flat, 2 * samples, f"pybench {variants}x{samples}", args.repeats, not args.no_torch, scores_of=g))


if __name__ == "__main__":
    main()
