// sweep_flat.hip — instantiations and launcher of the LDS-staged flat-tile route (sweep_flat_kernels.hpp): packed biallelic matrices with
// nothing missing whose rows are at most 32 vectors (4 096 columns).
#include "abi_internal.hpp"
#include "sweep_grid.hpp"
#include "sweep_flat_kernels.hpp"

using namespace fmh;

namespace fmhi {
namespace {

// LDS a workgroup's tile images take: waves x slots x nvec KiB (+ slack for the padded reads of the last row)
inline size_t flat_smem(uint32_t nvec, int slots) { return (size_t)kFlatWaves * slots * nvec * 1024u + kFlatLdsSlack; }

// the register-staged variant: one tile image per wave in LDS, the next tile in flight in registers
template <int P, int MODE, int NVMAX>
int launch_flat_rs(const SweepArgs& args_in, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  auto kern = sweep_kernel_flat_rs<P, MODE, NVMAX>;
  const uint32_t nvec = args_in.mv.nvec;
  static thread_local OccupancyCache cache;  // keyed by the row's vectors
  const size_t smem = flat_smem(nvec, 1);
  if (smem > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  int occ = 0;
  FMH_TRY(cached_occupancy(kern, kFlatBlock, smem, 8, true, cache, nvec, &occ));
  if (occ < 1) return fail(FMH_ERR_UNSUPPORTED, "a tile of %u vectors does not fit the LDS of the flat-tile route", nvec);
  SweepArgs args = args_in;
  args.flat_slots = 0;
  const size_t ntiles = (args.row_count + kTileRows - 1) / kTileRows;
  const size_t blocks = persistent_grid(occ, args.row_count, kFlatWaves, ctx);
  int depth = (int)options().flat_defer.load();
  if (depth < 1) {  // by the tiles a wave sweeps: short launches keep the undeferred order
    const size_t rounds = (ntiles + blocks * kFlatWaves - 1) / (blocks * kFlatWaves);
    depth = rounds >= 16 ? kFlatDeferMax : rounds >= 8 ? 4 : 1;
  }
  args.flat_defer = depth > flat_defer_max<P>() ? flat_defer_max<P>() : depth;
  return timed_launch(kern, blocks, kFlatBlock, smem, st, ctx, args, grid_out);
}

template <int P, int MODE, int NVMAX>
int launch_flat(const SweepArgs& args_in, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  if (options().flat_slots.load() == 0) return launch_flat_rs<P, MODE, NVMAX>(args_in, st, ctx, grid_out);  // FMH_FLAT_SLOTS = 1 | 2: the LDS-DMA variants
  auto kern = sweep_kernel_flat<P, MODE, NVMAX>;
  const uint32_t nvec = args_in.mv.nvec;
  static thread_local int cached_occ[64][2];
  static thread_local uint32_t cached_nvec[64];
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (cached_nvec[dev] != nvec) {
    for (int slots = 1; slots <= 2; ++slots) {
      const size_t smem = flat_smem(nvec, slots);
      int occ = 0;
      if (smem <= 160 * 1024 - 8 * 1024) {
        if (smem > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, kFlatBlock, smem));
      }
      if (occ > 8) occ = 8;  // the partial vectors hold 8 workgroups per CU
      cached_occ[dev][slots - 1] = occ;
    }
    cached_nvec[dev] = nvec;
  }
  SweepArgs args = args_in;
  // Tile images per wave.  Two slots keep a DMA in flight through the whole round of a wave, one slot leaves more waves resident.
  int slots = (int)options().flat_slots.load();
  if (slots != 1 && slots != 2) slots = cached_occ[dev][1] * kFlatWaves >= 8 ? 2 : 1;
  if (cached_occ[dev][slots - 1] < 1) slots = 1;
  int occ = cached_occ[dev][slots - 1];
  if (occ < 1) return fail(FMH_ERR_UNSUPPORTED, "a tile of %u vectors does not fit the LDS of the flat-tile route", nvec);
  args.flat_slots = slots;
  const size_t smem = flat_smem(nvec, slots);
  if (smem > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  return timed_launch(kern, persistent_grid(occ, args.row_count, kFlatWaves, ctx), kFlatBlock, smem, st, ctx, args, grid_out);
}

template <int P, int MODE>
int launch_nv(const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (a.mv.nvec <= 8) return launch_flat<P, MODE, 8>(a, st, ctx, grid);
  if (a.mv.nvec <= 20) return launch_flat<P, MODE, 20>(a, st, ctx, grid);
  return launch_flat<P, MODE, kFlatMaxVec>(a, st, ctx, grid);
}

}  // namespace

// packed rows of at most kFlatMaxVec vectors, biallelic, nothing missing; a.mask_flat set
int launch_sweep_flat(int P, int mode, const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (a.mv.nvec < 1 || a.mv.nvec > (uint32_t)kFlatMaxVec || !a.mask_flat || a.mv.pitch != (size_t)a.mv.nvec * 16)
    return fail(FMH_ERR_INVALID, "the flat-tile route takes packed rows of 1..%d vectors with pitch = 16 x vectors", kFlatMaxVec);
#define ROW(PV, MODEV) if (P == PV && mode == (MODEV)) return launch_nv<PV, MODEV>(a, st, ctx, grid);
  FMH_FLAT_BUILDS(ROW)
#undef ROW
  return fail(FMH_ERR_UNSUPPORTED, "no flat-tile sweep kernel for %d groups in mode %d", P, mode);
}

}  // namespace fmhi
