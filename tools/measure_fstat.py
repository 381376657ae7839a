#!/usr/bin/env python3
"""Development measurement of the f-statistics' moment kernel (fmh_fstat_moments) beside what the library offered before it for COUNTING
the same groups: fmh_population_summaries with its two per-site u32 tracks, in batches of at most eight groups, on the same matrix in the
same process.  That sweep reads the same planes once per batch and is what a user had to run (and then multiply on the host) before the
moments existed, so it is the yardstick; no ratio is fixed in advance.

Cohort: fmh_matrix_generate, complete and biallelic, allele frequencies skewed to rare alleles, packed.  Groups: G = 2, 4, 8 and 26 disjoint
populations, contiguous and (nearly) equal, covering every column.  Blocks: 2 000 equal row ranges.  Optionally (--item-rows, --mask-bytes)
the same under other FMH_FSTAT_ITEM_ROWS / FMH_FSTAT_LDS_MASK_BYTES values.

Per case: the library's HIP-event kernel time (fmh_timing_read) and the wall time of the whole call (which includes building and uploading
the mask entries and the item table and zero-filling the moments), best of --repeats after one warm-up, and the same two figures summed over
the yardstick's batches.  Before anything is timed the table is checked: every row accounted for in every block, the usable rows equal to
the rows the summaries sweep could call, and the whole-matrix call equal to the sum of the blocks.

Needs a GPU.  One JSON line per case to stdout and to profiles/fstat/measure_fstat.jsonl (or --out).
Default shape: 10 000 000 sites x 5 000 haplotypes; `tools/measure_fstat.py 1000000x5000` for others."""
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
from measure_sfs import device_cohort, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="SITESxHAPLOTYPES")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--groups", default="2,4,8,26")
    ap.add_argument("--item-rows", default="", help="comma-separated FMH_FSTAT_ITEM_ROWS values to time besides the default")
    ap.add_argument("--mask-bytes", default="", help="comma-separated FMH_FSTAT_LDS_MASK_BYTES values to time besides the default (1 = global memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fstat", "measure_fstat.jsonl"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes] or [(10_000_000, 5000)]
    lib = _abi.load()
    _abi.check(lib.fmh_timing_enable(1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:

        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for sites, n in shapes:
            dm = device_cohort(sites, n, seed=sites + n)
            edges = np.linspace(0, sites, args.blocks + 1).astype(np.uint64)
            blocks = np.ascontiguousarray(np.stack([edges[:-1], edges[1:]], axis=1))
            plane_bytes = sites * ((n + 127) // 128 * 16)
            for G in [int(v) for v in args.groups.split(",") if v]:
                masks = np.zeros((G, n), dtype=np.uint8)
                for g, part in enumerate(np.array_split(np.arange(n), G)):
                    masks[g, part] = 1
                width = device.fstat_moment_count(G)

                # ---- the yardstick: the summaries sweep with its per-site tracks, the same groups in batches of eight
                yard_kernel = yard_wall = 0.0
                uncallable = None
                for first in range(0, G, 8):
                    g = device.Groups(dm, masks[first:first + 8])
                    tracks = [device.DeviceBuffer(dm.device, 4 * g.n_groups * sites) for _ in range(2)]
                    totals = (_abi.PopTotals * g.n_groups)()
                    kernel, wall = timed(lambda: _abi.check(lib.fmh_population_summaries(dm._h, g._h, 0, sites, device.FORMULA_SUMMARY, tracks[0].ptr,
                                                                                          tracks[1].ptr, totals, None)), args.repeats)
                    yard_kernel += kernel
                    yard_wall += wall
                    if uncallable is None:
                        uncallable = int(totals[0].uncallable_sites)
                    for t in tracks:
                        t.free()
                    g.close()

                # ---- checks before timing
                got = device.fstat_moments(dm, masks, blocks)
                whole = device.fstat_moments(dm, masks)
                widths = (blocks[:, 1] - blocks[:, 0]).astype(np.uint64)
                ok = (np.array_equal(got.moments[:, 0] + got.multiallelic + got.incomplete, widths)
                      and int(got.moments[:, 0].sum()) == sites - uncallable
                      and np.array_equal(got.moments.sum(axis=0), whole.moments[0]))
                del got, whole

                def case(label):
                    table = device.DeviceBuffer(dm.device, 8 * width * len(blocks))
                    call = lambda: _abi.check(lib.fmh_fstat_moments(dm._h, masks.ctypes.data_as(C.c_void_p), G, blocks.ctypes.data_as(C.c_void_p),  # noqa: E731
                                                                    len(blocks), table.ptr, None, None))
                    kernel, wall = timed(call, args.repeats)
                    table.free()
                    emit({"case": f"{sites}x{n} {label}", "sites": sites, "haplotypes": n, "groups": G, "blocks": len(blocks), "slice_u64": width,
                          "checks_pass": bool(ok), "item_rows": _abi.get_option("FMH_FSTAT_ITEM_ROWS") or device.FSTAT_DEFAULT_ITEM_ROWS,
                          "lds_mask_bytes": _abi.get_option("FMH_FSTAT_LDS_MASK_BYTES") or device.FSTAT_DEFAULT_LDS_MASK_BYTES,
                          "fstat_kernel_ms": kernel, "fstat_call_wall_ms": wall, "plane0_gb_per_s_at_kernel_ms": plane_bytes / (kernel * 1e-3) / 1e9,
                          "summaries_batches": (G + 7) // 8, "summaries_kernel_ms": yard_kernel, "summaries_call_wall_ms": yard_wall,
                          "fstat_kernel_over_summaries_kernel": kernel / yard_kernel})

                case(f"moments of {G} disjoint populations, {len(blocks)} blocks")
                for value in [v for v in args.item_rows.split(",") if v]:
                    with _abi.options(FMH_FSTAT_ITEM_ROWS=value):
                        case(f"moments of {G} disjoint populations, item rows {value}")
                for value in [v for v in args.mask_bytes.split(",") if v]:
                    with _abi.options(FMH_FSTAT_LDS_MASK_BYTES=value):
                        case(f"moments of {G} disjoint populations, mask bytes {value}")
            dm.close()


if __name__ == "__main__":
    main()
