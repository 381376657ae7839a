#!/usr/bin/env python3
"""Development measurement of the admixture step (fmh_admix_create, fmh_admix_step): per cohort the image build (the larger span of HIP
events inside fmh_admix_create, fmh_timing_read_minmax), and per K the stages of one EM step by HIP events inside the library
(fmh_timing_read_admix: the padded state, the step kernel, the reduce) with and without the log-likelihood, best of --repeats after a warm-up;
the issued-MFMA TFLOP/s of the step kernel - (2 ceil(K / 4) + 16) MFMAs of 2 048 flops per 16 x 16 tile - against the 78.6 TFLOP/s f64 peak;
one accelerated cycle (three device steps through device.admix_step, which copies the state up and down, and fmh_admix_accelerate on the
host) by the wall clock; and in the same process the same step written with torch in f64 on the materialised dosage matrix (torch is only
this tool's yardstick, never a dependency of the library), against which Q' and F' are checked.

Needs a GPU.  One JSON line per (case, K) to stdout and to profiles/admix/measure_admix.jsonl (or the path given with --out).
Cases: SAMPLESxROWS[m] (m = about 2 % of the genotypes missing), default 2500x200000 2500x200000m; K = 2 4 8 16."""
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

PEAK_F64_MATRIX_TFLOPS = 78.6
EPS = 1e-5


def device_cohort(samples, rows, seed, missing, populations=5, scale=0.08):
    """tools/measure_grm.py's cohort; returns (matrix, genotype codes [rows][samples] uint8: 0, 1, 2, 3 = not called)."""
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=rows)
    thr = np.stack([np.clip(base + rng.normal(0.0, scale, size=rows), 0.001, 0.999) for _ in range(populations)])
    n = 2 * samples
    dm = device.DeviceMatrix.alloc(rows, samples, 2, missing, 1)
    dm.generate(seed, 0, (thr * float(1 << 24)).astype(np.uint32), (np.arange(n) * populations // n).astype(np.uint8), int(0.01 * (1 << 24)) if missing else 0)
    data, words = dm.download()
    data = data.reshape(rows, n)
    code = (data[:, 0::2] + data[:, 1::2]).astype(np.uint8)
    if words is not None:
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[: rows * n].reshape(rows, n)
        code[(bits[:, 0::2] | bits[:, 1::2]) != 0] = 3
    del data, words
    dm.pack(release_bytes=True)
    return dm, code


def torch_step(code, usable, sites, q, f, repeats):
    """(best ms, q', f') of the step in torch f64 on the materialised dosages of the usable rows [m][n]."""
    import torch

    g8 = torch.from_numpy(code[usable]).cuda()
    cal = g8 <= 2
    g = torch.where(cal, g8, torch.zeros_like(g8)).to(torch.float64)
    del g8
    Q, F = torch.from_numpy(q).cuda(), torch.from_numpy(f).cuda()
    two_m = 2.0 * torch.from_numpy(sites.astype(np.float64)).cuda()[:, None]
    zero = torch.zeros((), dtype=torch.float64, device="cuda")

    def step():
        G = 1.0 - F
        u = torch.where(cal, g / (F @ Q.T), zero)
        v = torch.where(cal, (2.0 - g) / (G @ Q.T), zero)
        fa, gb = F * (u @ Q), G * (v @ Q)
        f_new = torch.clamp(fa / (fa + gb), EPS, 1.0 - EPS)
        q0 = torch.clamp(Q * (u.T @ F + v.T @ G) / two_m, EPS, 1.0 - EPS)
        return q0 / q0.sum(dim=1, keepdim=True), f_new

    out = step()
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = step()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    res = best, out[0].cpu().numpy(), out[1].cpu().numpy()
    del g, cal, out
    torch.cuda.empty_cache()
    return res


def measure(samples, rows, missing, ks, repeats, with_torch, out):
    lib = _abi.load()
    dm, code = device_cohort(samples, rows, samples + rows, missing)
    build = None
    image = None
    for i in range(repeats + 1):
        if image is not None:
            image.close()
        _abi.check(lib.fmh_timing_reset())
        image = device.AdmixImage(dm)
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _abi.check(lib.fmh_timing_read_minmax(C.byref(lo), C.byref(hi)))
        if i and (build is None or hi.value < build):
            build = hi.value
    dm.close()
    tiles = ((image.m + 127) // 128 * 8) * ((image.n + 15) // 16)
    for K in ks:
        q, f = device.admix_start(image.called[image.usable], image.allele_count[image.usable], image.n, K, 1)
        stages = {}
        got = None
        for logs in (True, False):
            best = None
            for i in range(repeats + 1):
                got = device.admix_step(image, q, f, loglik=logs)
                ms = (C.c_double * 3)()
                _abi.check(lib.fmh_timing_read_admix(ms))
                if i and (best is None or ms[1] < best[1]):
                    best = list(ms)
            stages[logs] = best
        t0 = time.perf_counter()
        s1 = device.admix_step(image, q, f)
        s2 = device.admix_step(image, s1[0], s1[1])
        qa, fa, alpha = device.admix_accelerate((q, f), s1[:2], s2[:2])
        device.admix_step(image, qa, fa)
        cycle_ms = (time.perf_counter() - t0) * 1e3
        flops = tiles * (2 * ((K + 3) // 4) + 16) * 2048.0
        row = {"case": f"{samples}x{rows}{'m' if missing else ''}", "samples": samples, "rows": rows, "usable_rows": image.m, "missing": missing, "k": K,
               "image_build_ms": build, "pad_ms": stages[True][0], "step_with_loglik_ms": stages[True][1], "step_without_loglik_ms": stages[False][1],
               "reduce_ms": stages[True][2], "accelerated_cycle_with_host_copies_ms": cycle_ms, "alpha": alpha,
               "issued_mfma_tflops": flops / (stages[False][1] * 1e-3) / 1e12,
               "fraction_of_peak": flops / (stages[False][1] * 1e-3) / 1e12 / PEAK_F64_MATRIX_TFLOPS, "item_rows_option": _abi.get_option("FMH_ADMIX_ITEM_ROWS")}
        if with_torch:
            ms, tq, tf = torch_step(code, image.usable, image.sample_sites, q, f, repeats)
            row["torch_f64_step_ms"] = ms
            row["time_over_torch"] = (stages[False][0] + stages[False][1] + stages[False][2]) / ms
            row["q_max_rel_err_vs_torch"] = float((np.abs(got[0] - tq) / tq).max())
            row["f_max_rel_err_vs_torch"] = float((np.abs(got[1] - tf) / tf).max())
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    image.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="SAMPLESxROWS, an m behind it for about 2 %% missing genotypes")
    ap.add_argument("--k", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admix", "measure_admix.jsonl"))
    args = ap.parse_args()
    cases = args.cases or ["2500x200000", "2500x200000m"]
    _abi.check(_abi.load().fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for case in cases:
            missing = case.endswith("m")
            samples, rows = (int(v) for v in case.rstrip("m").split("x"))
            measure(samples, rows, missing, args.k, args.repeats, not args.no_torch, out)


if __name__ == "__main__":
    main()
