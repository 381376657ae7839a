#!/usr/bin/env python3
"""Development measurement of the banded linkage-disequilibrium kernel (fmh_ld_band): per shape and core the HIP-event kernel time
(events inside the library, fmh_timing_read) as pair-bits per second - sites x band x haplotypes bits ANDed and counted - against two
yardsticks:

  * the VALU bound: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz lane-operations per second (the chip's figures) at two lane-operations
    (v_and_b32 + v_bcnt_u32_b32) per 32 pair-bits - times four when calls can be missing, which counts four products per pair;
  * torch in the same process: the same counts as matrix products - the bits unpacked to fp16 0/1, one torch.mm per block of `band`
    rows against the block's band + band partner rows (block-diagonal; twice the pairs the band needs), four products when calls can be
    missing.  torch is only this tool's yardstick, never a dependency of the library.

Two kernel times per case: with only the threshold bits written (what fmh_ld_prune runs) and with r^2 as well (8 bytes per pair).
A corner of the result is checked against tests/ld_ref.py before anything is timed.

Needs a GPU.  One JSON line per case to stdout and to profiles/ld/measure_ld.jsonl (or --out).
Default shapes: 200 000 sites x 5 000 haplotypes at band 128, 512 and 1 000, both cores; `tools/measure_ld.py 50000x2000x256` for others."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ferromic_amd import _abi, device  # noqa: E402
from tests import ld_ref  # noqa: E402

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
VALU_BOUND_PAIR_BITS_PER_S = VALU_LANE_OPS_PER_S / 2.0 * 32.0


def device_cohort(n, sites, seed, missing):
    """A five-population cohort written by the library's generator straight into device memory, packed; (matrix, host alleles, host called)."""
    rng = np.random.default_rng(seed)
    base = rng.beta(0.8, 0.8, size=sites)
    thr = np.stack([np.clip(base + rng.normal(0.0, 0.08, size=sites), 0.001, 0.999) for _ in range(5)])
    dm = device.DeviceMatrix.alloc(sites, n // 2, 2, missing, 1)
    dm.generate(seed, 0, (thr * float(1 << 24)).astype(np.uint32), (np.arange(n) * 5 // n).astype(np.uint8), int(0.03 * (1 << 24)) if missing else 0)
    data, words = dm.download()
    called = None
    if words is not None:
        called = ~np.unpackbits(words.view(np.uint8), bitorder="little")[: sites * n].astype(bool).reshape(sites, n)
    dm.pack(release_bytes=True)
    return dm, data.reshape(sites, n), called


def kernel_ms(dm, band, want, repeats):
    lib = _abi.load()
    best = None
    for i in range(repeats + 1):  # the first call warms up
        _abi.check(lib.fmh_timing_reset())
        device_call(dm, band, want)
        total, launches = C.c_double(), C.c_uint64()
        _abi.check(lib.fmh_timing_read(C.byref(total), C.byref(launches)))
        if i:
            best = total.value if best is None else min(best, total.value)
    return best


def device_call(dm, band, want):
    """fmh_ld_band into device buffers that are not copied back."""
    rows, words = dm.variants, (band + 31) // 32
    bufs = {"over": device.DeviceBuffer(dm.device, 4 * rows * words)}
    if "r2" in want:
        bufs["r2"] = device.DeviceBuffer(dm.device, 8 * rows * band)
    out = _abi.LdBandOut(bufs["r2"].ptr if "r2" in bufs else None, None, None, bufs["over"].ptr)
    _abi.check(_abi.load().fmh_ld_band(dm._h, None, 0, rows, rows, band, 0.2, C.byref(out), None, None, None))
    for b in bufs.values():
        b.free()


def torch_ms(alleles, called, band, repeats):
    import torch

    a = torch.from_numpy(alleles).cuda().to(torch.float16)
    mats = [(a, a)]
    if called is not None:
        c = torch.from_numpy(called).cuda().to(torch.float16)
        a = a * c
        mats = [(a, a), (a, c), (c, a), (c, c)]
    rows = a.shape[0]

    def sweep():
        for i0 in range(0, rows, band):
            i1, j1 = min(i0 + band, rows), min(i0 + 2 * band, rows)
            for x, y in mats:
                torch.mm(x[i0:i1], y[i0:j1].T)

    sweep()
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sweep()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1)
        best = t if best is None else min(best, t)
    del a, mats
    torch.cuda.empty_cache()
    return best


def check_corner(dm, alleles, called, band):
    rows = min(192, dm.variants)
    pend = min(rows + band, dm.variants)
    b = min(band, 130)
    got = device.ld_band(dm, None, b, 0.2, 0, rows, pend)
    ref = ld_ref.band(alleles[:pend], None if called is None else called[:pend], None, 0, rows, pend, b, 0.2)
    same = (got.r2.view(np.uint64) == ref["r2"].view(np.uint64)) | (np.isnan(got.r2) & np.isnan(ref["r2"]))
    return bool(same.all() and np.array_equal(got.n_ab, ref["n_ab"]) and np.array_equal(got.over, ref["over"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPESxBAND")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld", "measure_ld.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(200_000, 5000, b) for b in (128, 512, 1000)]
    _abi.check(_abi.load().fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    cohorts = {}
    with open(args.out, "a") as out:
        for missing in (False, True):
            for sites, n, band in shapes:
                key = (sites, n, missing)
                if key not in cohorts:
                    for old in cohorts.values():
                        old[0].close()
                    cohorts.clear()
                    cohorts[key] = device_cohort(n, sites, seed=sites + n, missing=missing)
                dm, alleles, called = cohorts[key]
                ok = check_corner(dm, alleles, called, band)
                pair_bits = float(sites) * band * n
                bits_ms = kernel_ms(dm, band, ("over",), args.repeats)
                r2_ms = kernel_ms(dm, band, ("over", "r2"), args.repeats)
                products = 4 if missing else 1
                row = {"case": f"{sites}x{n} band {band} {'missing' if missing else 'complete'}", "sites": sites, "haplotypes": n, "band": band,
                       "core": "MISSING" if missing else "complete", "corner_matches_oracle": ok, "pair_bits": pair_bits,
                       "kernel_ms_bits_only": bits_ms, "kernel_ms_with_r2": r2_ms, "pair_bits_per_s_bits_only": pair_bits / (bits_ms * 1e-3),
                       "pair_bits_per_s_with_r2": pair_bits / (r2_ms * 1e-3), "valu_bound_pair_bits_per_s": VALU_BOUND_PAIR_BITS_PER_S / products,
                       "fraction_of_valu_bound_bits_only": pair_bits / (bits_ms * 1e-3) / (VALU_BOUND_PAIR_BITS_PER_S / products)}
                if not args.no_torch:
                    t = torch_ms(alleles, called, band, args.repeats)
                    row.update({"torch_fp16_block_mm_ms": t, "torch_pair_bits_per_s": pair_bits / (t * 1e-3), "kernel_time_over_torch": bits_ms / t})
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
