// sweep_tiled.hip — instantiations and launcher of the sweep over the tile-transposed plane image (sweep_tiled_kernels.hpp): packed biallelic
// matrices with nothing missing that hold the image (fmh_matrix::p0t), one or two groups, every mode that may derive a group.
#include "abi_internal.hpp"
#include "sweep_tiled_kernels.hpp"

using namespace fmh;

namespace fmhi {
namespace {

template <int P, int MODE, int C, int HB>
int launch_tiled(const SweepArgs& args, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  auto kern = sweep_kernel_tiled<P, MODE, C, HB>;
  static thread_local int cached_occ[64];
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (cached_occ[dev] == 0) {
    int occ = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, kBlock, 0));
    if (occ < 1) occ = 1;
    if (occ > 8) occ = 8;
    cached_occ[dev] = occ;
  }
  int occ = cached_occ[dev];
  if (const int env_occ = (int)options().max_occ.load(); env_occ > 0 && occ > env_occ) occ = env_occ;
  const size_t ntiles = (args.row_count + kTileRows - 1) / kTileRows;
  size_t blocks = (ntiles + kWavesPerBlock - 1) / kWavesPerBlock;
  size_t cap = (size_t)ctx.cus * occ;
  if (const long long v = options().grid_per_cu.load(); v > 0) cap = (size_t)ctx.cus * (size_t)v;
  if (const long long v = options().grid_blocks.load(); v > 0) cap = (size_t)v;
  if (blocks > cap) blocks = cap;  // persistent grid
  if (blocks > (size_t)ctx.max_grid) blocks = ctx.max_grid;
  if (blocks < 1) blocks = 1;
  if (ctx.timing) HIP_TRY(hipEventRecord(ctx.ev0, st));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kBlock), 0, st, args);
  HIP_TRY(hipGetLastError());
  if (ctx.timing) HIP_TRY(hipEventRecord(ctx.ev1, st));
  *grid_out = (int)blocks;
  return FMH_OK;
}

// The batch (2 x HB vectors): the deepest of 20, 10 and 4 that pads the window by at most a quarter, else 4.  A window of one batch has every
// one of its loads in flight from the previous tile's last half on (C4's 20 vectors: one batch).
template <int P, int MODE, int C>
int launch_batch(const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if constexpr (C == 0) return launch_tiled<P, MODE, 0, 1>(a, st, ctx, grid);  // nothing is counted: no vector is read
  else {
    const size_t w = a.mv.nvec;
    const long long want = options().tiled_batch.load();  // FMH_TILED_BATCH = 10 | 5 | 2: that half batch (measurements)
    if (want == 10) return launch_tiled<P, MODE, C, 10>(a, st, ctx, grid);
    if (want == 5) return launch_tiled<P, MODE, C, 5>(a, st, ctx, grid);
    if (want == 2) return launch_tiled<P, MODE, C, 2>(a, st, ctx, grid);
    if (round_up(w, 20) * 4 <= w * 5) return launch_tiled<P, MODE, C, 10>(a, st, ctx, grid);
    if (round_up(w, 10) * 4 <= w * 5) return launch_tiled<P, MODE, C, 5>(a, st, ctx, grid);
    return launch_tiled<P, MODE, C, 2>(a, st, ctx, grid);
  }
}

template <int P, int MODE>
int launch_counted(const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (a.derived_group >= 0) return launch_batch<P, MODE, P - 1>(a, st, ctx, grid);
  return launch_batch<P, MODE, P>(a, st, ctx, grid);
}

}  // namespace

bool tiled_route_builds(int P, int mode) {
  if (mode == kModeSummary) return P == 1 || P == 2;
  if (mode == (kModeSummary | kModeHudson)) return P == 2;
  if (mode == (kModeSummary | kModeDiversity)) return P == 1 || P == 2;
  if (mode == (kModeSummary | kModeHudson | kModeDiversity)) return P == 2;
  return false;
}

// a.mv.data = the image at the window's first vector, a.mv.nvec = the window's vectors, a.mv.pitch = 16 x the vectors of a whole row,
// a.mask_bits at the window's first vector; a.derived_group / a.row_alt as on the row-major routes
int launch_sweep_tiled(int P, int mode, const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (a.mv.nvec < 1 || a.mv.pitch < (size_t)a.mv.nvec * 16 || a.derived_group >= P || (a.derived_group >= 0 && !a.row_alt))
    return fail(FMH_ERR_INVALID, "the tiled route takes a window of 1..pitch / 16 vectors and a derived group with its row totals");
#define CASE(PV, MODEV) return launch_counted<PV, MODEV>(a, st, ctx, grid)
  if (mode == kModeSummary) {
    if (P == 1) CASE(1, kModeSummary);
    if (P == 2) CASE(2, kModeSummary);
  } else if (mode == (kModeSummary | kModeHudson)) {
    if (P == 2) CASE(2, kModeSummary | kModeHudson);
  } else if (mode == (kModeSummary | kModeDiversity)) {
    if (P == 1) CASE(1, kModeSummary | kModeDiversity);
    if (P == 2) CASE(2, kModeSummary | kModeDiversity);
  } else if (mode == (kModeSummary | kModeHudson | kModeDiversity)) {
    if (P == 2) CASE(2, kModeSummary | kModeHudson | kModeDiversity);
  }
#undef CASE
  return fail(FMH_ERR_UNSUPPORTED, "no tiled sweep kernel for %d groups in mode %d", P, mode);
}

}  // namespace fmhi
