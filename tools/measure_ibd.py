#!/usr/bin/env python3
"""Development measurement of the IBD-segment scan (fmh_ibd_scan) beside the host twin fmh_ibd_scan_host on the host's cores, and the sweep
over the number of row blocks that DESIGN.md section 3.22 records.  No speed figure is fixed in advance.

Cohort: fmh_matrix_generate, diploid, biallelic, allele frequencies skewed to rare alleles, packed; once complete and once with about 1 % of
the genotypes uncalled (tools/measure_kinship.py's cohorts).  Both modes; the filters are IBIS's marker count with the lengths loosened to
the cohort (row numbers as positions): the kernel's work per word depends on the discordant rows, not on the filters, but a run that is
rejected by its site count costs no position fetch, as in real use.

Per cohort and mode, the library's HIP-event kernel time (fmh_timing_read: the whole call - memset of the bit image, flags, states, pair
and stitch kernels) and the wall time of the call, best of --repeats after one warm-up, tables only; pair-words per second (pairs x
ceil(rows / 64)).  The three kernels separately come from a kernel trace of `--child ... --scan-only` in a run of its own, not from this
tool.  Then the block sweep: FMH_IBD_ITEM_ROWS forced so that the rows fall into 1, 2, 4, 8 and 16 blocks, at the cohort's sample count and
at --sweep-samples, mode IBD1: the default rule (ibd_host.hpp: kIbdItemsPerWorkgroup) is judged by it.  The host twin runs over
--host-rows rows x --host-samples samples of a second cohort of the same recipe, the samples split into --host-threads blocks whose
pairs one thread each scans, and is scaled by the ratio of pairs x rows: its time is linear in both.  Before anything is timed the device's tables over that
cohort are compared with the twin's.

Needs a GPU.  Every cohort is measured by a child process of its own under a time limit (--step-seconds); after a child that fails or runs
out of time nothing more is started.  One JSON line per case to stdout and to profiles/ibd/measure_ibd.jsonl (or --out).
Default shape: 1 000 000 sites x 5 000 haplotypes (2 500 samples): it fits the default budget (FMH_IBD_BUDGET_BYTES = 4 GiB);
`tools/measure_ibd.py 2000000x5000` for others."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def dosages_of(dm, n):
    """[variants][n] uint8 dosages (3 = not called) of a matrix's first n samples, from its download."""
    data, words = dm.download()
    x = data.reshape(dm.variants, dm.columns)
    a, b = x[:, 0::2], x[:, 1::2]
    ok = (a <= 1) & (b <= 1)
    if words is not None:
        miss = np.unpackbits(words.view(np.uint8), bitorder="little")[: x.size].reshape(x.shape).astype(bool)
        ok &= ~(miss[:, 0::2] | miss[:, 1::2])
    return np.ascontiguousarray(np.where(ok, a + b, 3).astype(np.uint8)[:, :n])


def host_twin_ms(device, d, params, threads):
    """The twin on `threads` threads: the samples are split into `threads` blocks and each thread scans every pair inside its block (one
    call on a contiguous copy of its columns).  Returns (wall ms, pairs scanned); the caller scales by pairs x rows."""
    n = d.shape[1]
    chunks = [c for c in np.array_split(np.arange(n), threads) if c.size > 1]
    copies = [np.ascontiguousarray(d[:, c]) for c in chunks]
    pairs = sum(c.size * (c.size - 1) // 2 for c in chunks)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=len(chunks)) as pool:   # ctypes releases the GIL around the call
        list(pool.map(lambda s: device.ibd_scan_host(s, params), copies))
    return (time.perf_counter() - t0) * 1e3, pairs


def measure(sites, haplotypes, missing, repeats, host_rows, host_samples, host_threads, sweep_samples, scan_only):
    """One cohort, in this process; yields one dict per case."""
    from ferromic_amd import _abi, device
    from measure_kinship import cohort
    from measure_sfs import timed

    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    n = haplotypes // 2
    words = -(-sites // 64)
    dm = cohort(sites, n, missing, seed=sites + n)
    label = f"{sites}x{haplotypes} " + ("about 1 % of the genotypes uncalled" if missing else "complete")

    def params_of(mode):
        return device.ibd_params(mode=mode, min_sites=436, min_length=436, max_gap=0, max_bp_per_site=0)

    # ---- check before timing, and the host twin's time: a second cohort of the same recipe
    host = {}
    if not scan_only:
        rows, m = min(sites, host_rows), min(n, host_samples)
        small = cohort(rows, n, missing, seed=rows + n + 1)
        d = dosages_of(small, m)
        for mode in (device.IBD1, device.IBD2):
            loose = device.ibd_params(mode=mode, min_sites=20, min_length=1, max_gap=0, max_bp_per_site=0)
            got = device.ibd_scan(small, loose, n_samples=m)
            twin = device.ibd_scan_host(d, loose)
            ok = all(np.array_equal(twin.tables[name], got.tables[name]) for name in device.IBD_TABLES)
            ms, pairs = host_twin_ms(device, d, params_of(mode), host_threads)
            host[mode] = dict(checks_pass=ok, segments_in_the_checked_rows=int(np.triu(got.tables["n_segments"], 1).sum()), host_twin_rows=rows,
                              host_twin_pairs=pairs, host_twin_threads=host_threads, host_twin_ms=ms)
        small.close()
        del d

    bufs = {name: device.DeviceBuffer(dm.device, 8 * n * n) for name in device.IBD_TABLES}
    out = _abi.IbdOut(*[bufs[name].ptr for name in device.IBD_TABLES])

    def scan(mode, samples):
        p = params_of(mode)
        return timed(lambda: _abi.check(lib.fmh_ibd_scan(dm._h, None, samples, 0, sites, None, None, C.byref(p), C.byref(out), None, 0, None, None)), repeats)

    for mode in (device.IBD1, device.IBD2):
        kernel, wall = scan(mode, n)
        pair_words = n * (n - 1) // 2 * words
        r = {"case": f"{label}: fmh_ibd_scan, mode IBD{mode}, tables only, default blocks", "sites": sites, "haplotypes": haplotypes, "samples": n,
             "missing": missing, "mode": mode, "repeats": repeats, "kernel_ms": kernel, "call_wall_ms": wall, "pair_words": pair_words,
             "giga_pair_words_per_s": pair_words / (kernel * 1e-3) / 1e9 if kernel else None}
        if mode in host:
            h = host[mode]
            scaled = h["host_twin_ms"] * (n * (n - 1) // 2 * sites) / (h["host_twin_pairs"] * h["host_twin_rows"])
            r.update(h, host_twin_ms_scaled_to_all_pairs_and_rows=scaled, host_twin_scaled_over_kernel=scaled / kernel if kernel else None)
        yield r
    if scan_only:
        dm.close()
        return
    # ---- the block sweep, mode IBD1
    for samples in sorted({n, min(n, sweep_samples)}, reverse=True):
        for blocks in (1, 2, 4, 8, 16):
            item_rows = -(-words // blocks) * 64
            _abi.set_option("FMH_IBD_ITEM_ROWS", item_rows)
            try:
                kernel, wall = scan(device.IBD1, samples)
            finally:
                _abi.set_option("FMH_IBD_ITEM_ROWS", None)
            tiles = -(-samples // 32) * (-(-samples // 32) + 1) // 2
            yield {"case": f"{label}: block sweep, mode IBD1, {samples} samples, {blocks} blocks", "sites": sites, "samples": samples, "missing": missing,
                   "blocks": -(-sites // item_rows), "item_rows": item_rows, "tile_pairs": tiles, "items": tiles * -(-sites // item_rows),
                   "repeats": repeats, "kernel_ms": kernel, "call_wall_ms": wall}
        kernel, wall = scan(device.IBD1, samples)
        yield {"case": f"{label}: block sweep, mode IBD1, {samples} samples, default blocks", "sites": sites, "samples": samples, "missing": missing,
               "repeats": repeats, "kernel_ms": kernel, "call_wall_ms": wall}
    dm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=20_000)
    ap.add_argument("--host-samples", type=int, default=320)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--sweep-samples", type=int, default=600)
    ap.add_argument("--scan-only", action="store_true", help="the default-block scans only (for a kernel trace)")
    ap.add_argument("--step-seconds", type=int, default=300, help="time limit of one cohort's child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibd", "measure_ibd.jsonl"))
    ap.add_argument("--child", nargs=3, metavar=("SITES", "HAPLOTYPES", "MISSING"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        for r in measure(int(args.child[0]), int(args.child[1]), args.child[2] == "1", args.repeats, args.host_rows, args.host_samples, args.host_threads,
                         args.sweep_samples, args.scan_only):
            print(json.dumps(r), flush=True)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(1_000_000, 5000)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:  # a run replaces the file: one run per profile
        for sites, haplotypes in shapes:
            for missing in (False, True):
                cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--host-rows", str(args.host_rows), "--host-samples",
                       str(args.host_samples), "--host-threads", str(args.host_threads), "--sweep-samples", str(args.sweep_samples), "--child", str(sites),
                       str(haplotypes), "1" if missing else "0"] + (["--scan-only"] if args.scan_only else [])
                try:
                    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_seconds)
                except subprocess.TimeoutExpired:
                    print(f"measure_ibd: {sites}x{haplotypes} missing={missing} ran out of its {args.step_seconds} s: stopping", file=sys.stderr)
                    return 124
                lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
                for ln in lines:
                    print(ln, flush=True)
                    out.write(ln + "\n")
                out.flush()
                if res.returncode != 0:
                    print(res.stderr[-3000:], file=sys.stderr)
                    print(f"measure_ibd: the child of {sites}x{haplotypes} missing={missing} ended with status {res.returncode}: stopping", file=sys.stderr)
                    return res.returncode if res.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
