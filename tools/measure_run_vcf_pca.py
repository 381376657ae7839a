#!/usr/bin/env python3
"""run_vcf --pca at scale, and the pack / unpack kernels of fmh_pca_gram_sharded.  Needs a GPU.

Writes one JSON line per measurement to --out (default profiles/pca/run_vcf_pca.jsonl):
  * run_vcf on the synthetic VCF of tools/run_vcf_scale.py (default 200 000 sites x 5 000 haplotypes): three runs each of this build
    with --pca, this build without, and - with --parent-bin - another build of the binary on the same file with --pca (a build from
    before the feature ignores the flag); wall time and the [TIMING] lines, the `pca` stage split among them;
  * --devices 0,0 --pca with FERROMIC_SHARD_MIN_BYTES=1 against one device: on ONE GPU this is only the overhead of the sharded route
    (two half Grams one after the other on one GPU + the host rendezvous), not a speed-up of anything;
  * the pack / unpack kernels at n haplotypes (default 5 000): fmh_pca_gram_sharded on a one-rank RCCL communicator against
    fmh_pca_gram on the same input by wall clock, and the two kernels' own durations from `rocprofv3 --kernel-trace --stats` around a
    child process of this script (--kernels-child), with bytes/s against what they read and write.
"""

from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "ferromic_amd", "bin", "run_vcf")


def gram_case(n, m, seed=5):
    from tests import pca_ref as R

    rng = np.random.default_rng(seed)
    x = (rng.random((m, n)) < rng.uniform(0.1, 0.9, size=(m, 1))).astype(np.uint8)
    x[:, 0], x[:, n - 1] = 1, 0
    hi, lo = R.set_clear_values(x.sum(axis=1), n)
    return x, np.arange(m, dtype=np.uint64), hi, lo


def kernels_child(n, m, repeats):
    """What rocprofv3 traces: `repeats` sharded Grams on a one-rank RCCL communicator (pack -> ncclAllReduce -> unpack each)."""
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    x, kept, hi, lo = gram_case(n, m)
    dm = dev.DeviceMatrix.from_host(x, None, m, n // 2, 2, 1)
    comm = sharding.Comm.single(0)
    for _ in range(repeats):
        dev.pca_gram_sharded_device(comm, dm, kept, hi, lo)
    comm.close()
    dm.close()


def measure_kernels(n, m, repeats, out):
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    x, kept, hi, lo = gram_case(n, m)
    dm = dev.DeviceMatrix.from_host(x, None, m, n // 2, 2, 1)
    comm = sharding.Comm.single(0)
    wall = {"fmh_pca_gram": [], "fmh_pca_gram_sharded": []}
    for i in range(repeats + 1):
        for name, call in (("fmh_pca_gram", lambda: dev.pca_gram_device(dm, kept, hi, lo)), ("fmh_pca_gram_sharded", lambda: dev.pca_gram_sharded_device(comm, dm, kept, hi, lo))):
            t0 = time.perf_counter()
            buf = call()
            dt = time.perf_counter() - t0
            del buf
            if i:  # the first round warms the pool and RCCL up
                wall[name].append(dt * 1e3)
    comm.close()
    dm.close()
    tri_bytes, full_bytes = 4 * n * (n + 1), 8 * n * n
    line = {"what": "pack_unpack_kernels", "haplotypes": n, "kept_sites": m, "repeats": repeats, "wall_ms": wall,
            "sharded_minus_plain_ms_best": min(wall["fmh_pca_gram_sharded"]) - min(wall["fmh_pca_gram"]),
            "note": "one-rank RCCL communicator: the difference is pack + ncclAllReduce over one rank + unpack + the scratch block and events"}
    prof = tempfile.mkdtemp(prefix="pca_kernels_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
           "--kernels-child", "--haplotypes", str(n), "--kernel-sites", str(m), "--repeats", str(repeats)]
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line["rocprofv3_exit"] = res.returncode
        durations = {}
        for path in glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Kernel_Name", "")
                for key in ("pca_pack_triangle_kernel", "pca_unpack_triangle_kernel", "pca_gram_kernel"):
                    if key in name:
                        durations.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        moved = {"pca_pack_triangle_kernel": (tri_bytes, tri_bytes), "pca_unpack_triangle_kernel": (tri_bytes, full_bytes)}
        for key, us in durations.items():
            entry = {"calls": len(us), "best_us": min(us), "median_us": float(np.median(us))}
            if key in moved:
                entry["bytes_read"], entry["bytes_written"] = moved[key]
                entry["TB_per_s_at_best"] = sum(moved[key]) / (min(us) * 1e-6) / 1e12
                entry["fraction_of_8_TB_per_s"] = entry["TB_per_s_at_best"] / 8.0
            line[key] = entry
        if not durations:
            line["rocprofv3_stderr_tail"] = res.stderr[-600:]
    except (OSError, subprocess.TimeoutExpired) as exc:
        line["rocprofv3_error"] = str(exc)
    out.write(json.dumps(line) + "\n")
    out.flush()
    print(json.dumps(line))


def run_binary(binary, tmp, extra, env_extra, tag, out, run_index):
    cwd = os.path.join(tmp, f"cwd_{tag}_{run_index}")
    os.makedirs(cwd, exist_ok=True)
    cmd = [binary, "--vcf_folder", os.path.join(tmp, "vcfs"), "--reference", os.path.join(tmp, "ref.fa"), "--gtf", os.path.join(tmp, "ann.gtf"),
           "--config_file", os.path.join(tmp, "config.tsv"), "--output_file", os.path.join(cwd, "out", "results.csv"), "--fst"] + extra
    t0 = time.perf_counter()
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd, env=dict(os.environ, FERROMIC_TIMING="1", FERROMIC_PROGRESS="1", **env_extra), timeout=900)
    wall = time.perf_counter() - t0
    timing = {}
    for ln in res.stderr.splitlines():
        if ln.startswith("[TIMING]"):
            parts = ln[len("[TIMING]"):].rsplit(None, 1)
            timing[parts[0].strip()] = float(parts[1])
    pca_file = os.path.join(cwd, "pca_per_chr_outputs", "pca_chr_1.tsv")
    line = {"what": "run_vcf", "tag": tag, "run": run_index, "binary": os.path.relpath(binary, ROOT), "flags": extra, "env": env_extra, "exit": res.returncode,
            "wall_s": wall, "run_s": timing.get("run"), "pca_s": timing.get("pca"), "run_minus_pca_s": None if timing.get("run") is None else timing["run"] - timing.get("pca", 0.0),
            "timing": timing, "pca_file_bytes": os.path.getsize(pca_file) if os.path.exists(pca_file) else None,
            "pca_log": [ln for ln in res.stderr.splitlines() if "PCA" in ln or "complete data" in ln][:6]}
    out.write(json.dumps(line) + "\n")
    out.flush()
    print(json.dumps({k: line[k] for k in ("tag", "run", "exit", "wall_s", "run_s", "pca_s", "run_minus_pca_s", "pca_file_bytes")}))
    return line


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=2_500)
    ap.add_argument("--haplotypes", type=int, default=5_000, help="n of the pack / unpack measurement")
    ap.add_argument("--kernel-sites", type=int, default=8_192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-bin", default=None, help="a run_vcf binary of the commit before the feature (its own libferromic_hip.so beside it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca", "run_vcf_pca.jsonl"))
    ap.add_argument("--skip-run-vcf", action="store_true")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        kernels_child(args.haplotypes, args.kernel_sites, args.repeats)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        measure_kernels(args.haplotypes, args.kernel_sites, args.repeats, out)
        if args.skip_run_vcf:
            return 0
        from tools.run_vcf_scale import write_inputs

        tmp = tempfile.mkdtemp(prefix="run_vcf_pca_")
        t0 = time.perf_counter()
        _, _, _, vcf_bytes = write_inputs(tmp, args.sites, args.samples, 202_500)
        out.write(json.dumps({"what": "inputs", "sites": args.sites, "samples": args.samples, "vcf_bytes": vcf_bytes, "generate_s": time.perf_counter() - t0}) + "\n")
        # interleaved, so that a drift of the box hits every variant alike
        for i in range(args.runs):
            run_binary(BIN, tmp, ["--pca"], {}, "this_pca", out, i)
            run_binary(BIN, tmp, [], {}, "this_no_pca", out, i)
            if args.parent_bin:
                run_binary(os.path.abspath(args.parent_bin), tmp, ["--pca"], {}, "parent_pca_flag_ignored", out, i)
        for i in range(args.runs):
            run_binary(BIN, tmp, ["--pca", "--devices", "0,0"], {"FERROMIC_SHARD_MIN_BYTES": "1"}, "this_pca_devices_0_0_one_gpu", out, i)
        import shutil

        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
