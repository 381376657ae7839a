// sweep_grid.hpp — what the launchers of the persistent-grid sweeps share (sweep_launch.inc, sweep_flat.hip, sweep_tiled.hip,
// sweep_mfma.hip): the size of the grid from the kernel's occupancy and the grid options, and the launch between the timing events.  Two
// steps, because launch_one and launch_flat_rs choose their deferral depth from the grid between them.
#pragma once

#include "abi_internal.hpp"

namespace fmhi {

// One kernel instantiation's occupancy per device, with the key it was asked for (the dynamic LDS, or the row's vectors where that
// decides the LDS).  Each launcher template keeps its own `static thread_local` slot: one cache per instantiation and thread.
struct OccupancyCache {
  int occ[64];
  size_t key[64];
};

// The occupancy the grid is sized with: asked once per (device, key), capped at `ceiling`.  A kernel that does not fit (occupancy zero)
// counts as one workgroup per CU, or - `zero_is_error` - yields 0 and is asked again by the next launch.
template <class Kernel>
int cached_occupancy(Kernel kern, int block, size_t smem, int ceiling, bool zero_is_error, OccupancyCache& cache, size_t key, int* occ_out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (cache.occ[dev] == 0 || cache.key[dev] != key) {
    int occ = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, block, smem));
    if (occ < 1 && !zero_is_error) occ = 1;
    if (occ > ceiling) occ = ceiling;
    cache.occ[dev] = occ;
    cache.key[dev] = key;
  }
  *occ_out = cache.occ[dev];
  return FMH_OK;
}

// Workgroups of the persistent grid for `row_count` rows at `waves` tiles per workgroup and round: every tile its wave, at most the
// CUs x occupancy that are resident at once (equalising the tile rounds per workgroup was measured: fewer resident waves, slower).
// FMH_MAX_OCC is applied per launch, outside the cache: fmh_set_option may change it at any time (tools/ab_env.py alternates it).
inline size_t persistent_grid(int occ, size_t row_count, int waves, const LaunchCtx& ctx) {
  if (const int env_occ = (int)options().max_occ.load(); env_occ > 0 && occ > env_occ) occ = env_occ;
  const size_t ntiles = (row_count + fmh::kTileRows - 1) / fmh::kTileRows;
  size_t blocks = (ntiles + waves - 1) / waves;
  size_t cap = (size_t)ctx.cus * occ;
  if (const long long v = options().grid_per_cu.load(); v > 0) cap = (size_t)ctx.cus * (size_t)v;  // measurements
  if (const long long v = options().grid_blocks.load(); v > 0) cap = (size_t)v;                     // tests: many tile rounds on small inputs
  if (blocks > cap) blocks = cap;
  if (blocks > (size_t)ctx.max_grid) blocks = ctx.max_grid;
  if (blocks < 1) blocks = 1;
  return blocks;
}

template <class Kernel>
int timed_launch(Kernel kern, size_t blocks, int block, size_t smem, hipStream_t st, const LaunchCtx& ctx, const fmh::SweepArgs& args, int* grid_out) {
  if (ctx.timing) HIP_TRY(hipEventRecord(ctx.ev0, st));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(block), smem, st, args);
  HIP_TRY(hipGetLastError());
  if (ctx.timing) HIP_TRY(hipEventRecord(ctx.ev1, st));
  *grid_out = (int)blocks;
  return FMH_OK;
}

}  // namespace fmhi
