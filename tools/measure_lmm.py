#!/usr/bin/env python3
"""Development measurement of the mixed-model scan's device projections (fmh_lmm_projections): per shape the time of the call's kernels - the
basis and coefficient images and lmm_project_kernel, one span of HIP events inside the library (fmh_timing_read_minmax: the larger of the
call's two spans, the other being fmh_genotype_counts') - best of --repeats after a warm-up, the f64 TFLOP/s of the 2 K n rows flops of the
rotation against the 78.6 TFLOP/s matrix peak, and in the same process torch.mm in f64 of the same [K][n] x [n][rows] product on a
materialised, mean-imputed dosage matrix (torch is only this tool's yardstick, never a dependency of the library).  quad is checked
against the torch product over every row.  K = n, P = 1, L = 2.

Needs a GPU.  One JSON line per case to stdout and to profiles/lmm/measure_lmm.jsonl (or the path given with --out).
Cases: SAMPLESxROWS[m] (m = about 1 % of the genotypes missing), default 1000x150000 1000x150000m 2500x200000 2500x200000m."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ferromic_amd import _abi, device  # noqa: E402

PEAK_F64_MATRIX_TFLOPS = 78.6


def device_cohort(samples, rows, seed, missing, populations=5, scale=0.08):
    """tools/measure_grm.py's cohort; returns (matrix, genotype codes [rows][samples] uint8: 0, 1, 2, 3 = not called)."""
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=rows)
    thr = np.stack([np.clip(base + rng.normal(0.0, scale, size=rows), 0.001, 0.999) for _ in range(populations)])
    n = 2 * samples
    dm = device.DeviceMatrix.alloc(rows, samples, 2, missing, 1)
    dm.generate(seed, 0, (thr * float(1 << 24)).astype(np.uint32), (np.arange(n) * populations // n).astype(np.uint8), int(0.005 * (1 << 24)) if missing else 0)
    data, words = dm.download()
    data = data.reshape(rows, n)
    code = (data[:, 0::2] + data[:, 1::2]).astype(np.uint8)
    if words is not None:
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[: rows * n].reshape(rows, n)
        code[(bits[:, 0::2] | bits[:, 1::2]) != 0] = 3
    del data, words
    dm.pack(release_bytes=True)
    return dm, code


def torch_product(code, basis, weights, repeats):
    """(best ms of torch.mm(basis^T, X), quad [rows] from that product) with X [n][rows] the mean-imputed dosages in f64."""
    import torch

    g = torch.from_numpy(code).cuda()
    called = g <= 2
    c = called.sum(dim=1).to(torch.float64)
    a = torch.where(called, g, torch.zeros_like(g)).sum(dim=1, dtype=torch.int64).to(torch.float64)
    mu = torch.where(c > 0, a / torch.clamp(c, min=1.0), torch.zeros_like(c))
    x = torch.where(called, g.to(torch.float64), mu[:, None]).T.contiguous()  # [n][rows]
    del g, called
    bt = torch.from_numpy(np.ascontiguousarray(basis.T)).cuda()                # [K][n]
    t = torch.mm(bt, x)
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t = torch.mm(bt, x)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    quad = (torch.from_numpy(weights[0]).cuda()[:, None] * t * t).sum(dim=0).cpu().numpy()
    del t, x, bt
    torch.cuda.empty_cache()
    return best, quad


def measure(samples, rows, missing, repeats, with_torch):
    lib = _abi.load()
    dm, code = device_cohort(samples, rows, samples + rows, missing)
    rng = np.random.default_rng(samples)
    n = K = samples
    basis = np.linalg.qr(rng.normal(size=(n, K)))[0]
    weights, linear = rng.uniform(0.2, 1.0, size=(1, K)), rng.normal(size=(2, K))
    best, got = None, None
    for i in range(repeats + 1):
        _abi.check(lib.fmh_timing_reset())
        got = device.lmm_projections(dm, basis, weights, linear)
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _abi.check(lib.fmh_timing_read_minmax(C.byref(lo), C.byref(hi)))
        if i and (best is None or hi.value < best):
            best = hi.value
    flops = 2.0 * K * n * rows
    row = {"case": f"{samples}x{rows}{'m' if missing else ''}", "samples": samples, "rows": rows, "missing": missing, "components": K, "kernels_ms": best,
           "f64_tflops": flops / (best * 1e-3) / 1e12, "fraction_of_peak": flops / (best * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS,
           "item_rows_option": _abi.get_option("FMH_LMM_ITEM_ROWS")}
    dm.close()
    if with_torch:
        mm, quad = torch_product(code, basis, weights, repeats)
        row["torch_mm_f64_ms"] = mm
        row["torch_mm_f64_tflops"] = flops / (mm * 1e-3) / 1e12
        row["time_over_torch_mm"] = best / mm
        row["quad_max_rel_err_vs_torch"] = float((np.abs(got.quad[:, 0] - quad) / np.maximum(np.abs(quad), 1e-300)).max())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="SAMPLESxROWS, an m behind it for about 1 %% missing genotypes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmm", "measure_lmm.jsonl"))
    args = ap.parse_args()
    cases = args.cases or ["1000x150000", "1000x150000m", "2500x200000", "2500x200000m"]
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
