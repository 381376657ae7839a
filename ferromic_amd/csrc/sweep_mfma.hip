// sweep_mfma.hip — instantiations and launcher of the int8 matrix-core counting route (sweep_mfma_kernels.hpp).
#include "abi_internal.hpp"
#include "sweep_grid.hpp"
#include "sweep_mfma_kernels.hpp"

using namespace fmh;

namespace fmhi {
namespace {

template <int P, int MODE, int U>
int launch_mfma(const SweepArgs& args, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  auto kern = sweep_mfma_kernel<P, MODE, U>;
  static thread_local OccupancyCache cache;  // keyed by the dynamic LDS
  if (smem > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  int occ = 0;
  FMH_TRY(cached_occupancy(kern, kBlock, smem, 8, false, cache, smem, &occ));
  return timed_launch(kern, persistent_grid(occ, args.row_count, kWavesPerBlock, ctx), kBlock, smem, st, ctx, args, grid_out);
}

template <int P, int MODE>
int launch_u(int unroll, const SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (unroll == 2) return launch_mfma<P, MODE, 2>(a, smem, st, ctx, grid);
  return launch_mfma<P, MODE, 4>(a, smem, st, ctx, grid);
}

}  // namespace

// u8 rows, biallelic, nothing missing, P (padded) <= 4; a.unroll = K steps issued back to back (2 or 4), a.nvec_pad =
// mfma_mask_stride(nvec, unroll), smem = P * nvec_pad * 16
int launch_sweep_mfma(int P, int mode, const SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid) {
#define ROW(PV, MODEV) if (P == PV && mode == (MODEV)) return launch_u<PV, MODEV>(a.unroll, a, smem, st, ctx, grid);
  FMH_MFMA_BUILDS(ROW)
#undef ROW
  return fail(FMH_ERR_UNSUPPORTED, "no matrix-core sweep kernel for %d groups in mode %d", P, mode);
}

}  // namespace fmhi
