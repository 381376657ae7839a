// hap_launch.hpp — the threads per workgroup of the two haplotype kernels (hap.hip: one item = one window; ehh.hip: one item = one focal row
// and side).  One rule in one place, so the two units cannot drift apart; what every statistic shares is in stat_call.hpp.
#pragma once

#include <algorithm>

#include "abi_internal.hpp"

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

}  // namespace fmhi
