// hap_launch.hpp — what the statistics on the persistent grid share on the host side: the launch shape of the two haplotype kernels (hap.hip:
// one item = one window; ehh.hip: one item = one focal row and side) - threads per workgroup -, the size of the persistent grid (hap_grid:
// also fstat.hip, qc.hip, assoc.hip) and the event timer of a call's kernels (KernelTimer: qc.hip, assoc.hip).  One rule in one place, so the
// units cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_internal.hpp"
#include "hap_kernels.hpp"

namespace fmhi {

// Threads of a workgroup: the option, else by measurement (DESIGN.md sections 3.13 and 3.14, profiles/haplotypes/, profiles/ehh/).  With an item
// for every compute unit throughput counts, and at 2 500 and 5 000 members 256 threads - six to eight workgroups per CU - ran ahead of 512
// (1.1-1.6x) and of 1 024; with fewer items than compute units an item's own latency counts, and 512 (2 500 members) and 1 024 (5 000) ran
// ahead of 256 (1.3-1.9x).  The ends of both scales (64 threads for the smallest groups, more threads where LDS leaves a CU one or two
// workgroups) are not measured.
inline unsigned hap_pick_threads(uint32_t n, size_t n_items, int cus) {
  const long long opt = options().hap_threads.load(std::memory_order_relaxed);
  if (opt == 64 || opt == 256 || opt == 512 || opt == 1024) return (unsigned)opt;
  if (n <= 256) return 64;
  if (n_items < (size_t)std::max(cus, 1)) return n <= 1024 ? 256 : n <= 4096 ? 512 : 1024;
  return n <= 8192 ? 256 : n <= 16384 ? 512 : 1024;
}

// Workgroups of the persistent grid: the workgroups a CU holds by LDS and by its 2 048 thread slots (at most eight) - and, when
// `kernel_or_null` is given, by the kernel's registers as the runtime reports them: a workgroup beyond what is resident starts only when
// another has walked all its items, and then walks its own alone.  FMH_GRID_PER_CU / FMH_GRID_BLOCKS override; never more than the items.
// `lds_bytes` is the DYNAMIC LDS of the launch; a kernel that declares its LDS statically passes it as `static_lds_bytes` (the occupancy query
// reads it from the kernel itself and must not be told it twice).
inline int hap_grid(const void* kernel_or_null, unsigned threads, size_t lds_bytes, size_t n_items, int cus, size_t* grid_out, size_t static_lds_bytes = 0) {
  size_t per_cu = std::max<size_t>(1, std::min<size_t>({(size_t)8, fmh::kHapLdsPerCu / (lds_bytes + static_lds_bytes), (size_t)2048 / threads}));
  if (kernel_or_null) {
    int resident = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kernel_or_null, (int)threads, lds_bytes));
    if (resident > 0) per_cu = std::min(per_cu, (size_t)resident);
  }
  const long long opt_per_cu = options().grid_per_cu.load(std::memory_order_relaxed);
  if (opt_per_cu > 0) per_cu = (size_t)std::min<long long>(opt_per_cu, 32);
  size_t grid = (size_t)std::max(cus, 1) * per_cu;
  const long long opt_blocks = options().grid_blocks.load(std::memory_order_relaxed);
  if (opt_blocks > 0) grid = (size_t)std::min<long long>(opt_blocks, 1 << 20);
  *grid_out = std::min(grid, n_items);
  return FMH_OK;
}

// HIP events around a call's kernels when fmh_timing_enable is on, added to the library's kernel time after the synchronise (qc.hip, assoc.hip)
struct KernelTimer {
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool on = timing_enabled();
  ~KernelTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  int start(hipStream_t st) {
    if (!on) return FMH_OK;
    for (hipEvent_t& e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ev[0], st));
    return FMH_OK;
  }
  int stop(hipStream_t st) {
    if (on) HIP_TRY(hipEventRecord(ev[1], st));
    return FMH_OK;
  }
  int read() {
    if (!on) return FMH_OK;
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    timing_add(ms);
    return FMH_OK;
  }
};

}  // namespace fmhi
