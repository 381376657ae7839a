// sweep_tiled.hip — instantiations and launcher of the sweep over the tile-transposed plane image (sweep_tiled_kernels.hpp): packed biallelic
// matrices with nothing missing that hold the image (fmh_matrix::p0t), one or two groups, every mode that may derive a group.
#include "abi_internal.hpp"
#include "sweep_grid.hpp"
#include "sweep_tiled_kernels.hpp"

using namespace fmh;

namespace fmhi {
namespace {

template <int P, int MODE, int C, int HB>
int launch_tiled(const SweepArgs& args, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  auto kern = sweep_kernel_tiled<P, MODE, C, HB>;
  static thread_local OccupancyCache cache;  // no key: the kernel takes no dynamic LDS
  int occ = 0;
  FMH_TRY(cached_occupancy(kern, kBlock, 0, 8, false, cache, 0, &occ));
  return timed_launch(kern, persistent_grid(occ, args.row_count, kWavesPerBlock, ctx), kBlock, 0, st, ctx, args, grid_out);
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

// the table form: every counted group from the prefix counts and its edge vectors (at least one group is counted)
template <int P, int MODE, int C, int F, int HF>
int launch_prefix_pair(const SweepArgs& args, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  auto kern = sweep_kernel_tiled_prefix<P, MODE, C, F, HF>;
  static thread_local OccupancyCache cache;
  int occ = 0;
  FMH_TRY(cached_occupancy(kern, kBlock, 0, 8, false, cache, 0, &occ));
  return timed_launch(kern, persistent_grid(occ, args.row_count, kWavesPerBlock, ctx), kBlock, 0, st, ctx, args, grid_out);
}
// The formula pair of the launch picks the instantiation: one per formula where the population totals and the Hudson part share it (every
// sweep but the fused region sweep; only the Hudson part reads the second one), the region driver's two distinct pairs (dense or summary
// totals over the sparse Hudson set), and one that reads any other distinct pair from the arguments.
template <int P, int MODE, int C>
int launch_prefix(const SweepArgs& args, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  if constexpr (C < 1) return fail(FMH_ERR_INVALID, "the table form of the tiled route counts at least one group");
  else {
    const int f = args.formula, hf = args.hudson_formula_p1 ? args.hudson_formula_p1 - 1 : args.formula;
    if ((MODE & kModeHudson) == 0 || hf == f) {
      if (f == kFormulaSparse) return launch_prefix_pair<P, MODE, C, kFormulaSparse, kFormulaSparse>(args, st, ctx, grid_out);
      if (f == kFormulaDense) return launch_prefix_pair<P, MODE, C, kFormulaDense, kFormulaDense>(args, st, ctx, grid_out);
      if (f == kFormulaSummary) return launch_prefix_pair<P, MODE, C, kFormulaSummary, kFormulaSummary>(args, st, ctx, grid_out);
      return fail(FMH_ERR_INVALID, "unknown formula %d", f);
    }
    if constexpr ((MODE & kModeHudson) != 0 && (MODE & kModeDiversity) != 0) {
      if (f == kFormulaDense && hf == kFormulaSparse) return launch_prefix_pair<P, MODE, C, kFormulaDense, kFormulaSparse>(args, st, ctx, grid_out);
      if (f == kFormulaSummary && hf == kFormulaSparse) return launch_prefix_pair<P, MODE, C, kFormulaSummary, kFormulaSparse>(args, st, ctx, grid_out);
      return launch_prefix_pair<P, MODE, C, kFormulaRuntime, kFormulaRuntime>(args, st, ctx, grid_out);
    } else return fail(FMH_ERR_INVALID, "only the fused region sweep takes a Hudson formula of its own");
  }
}
template <int P, int MODE>
int launch_prefix_counted(const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (a.derived_group >= 0) return launch_prefix<P, MODE, P - 1>(a, st, ctx, grid);
  return launch_prefix<P, MODE, P>(a, st, ctx, grid);
}

}  // namespace

// a.mv.data = the image at the window's first vector, a.mv.nvec = the window's vectors, a.mv.pitch = 16 x the vectors of a whole row,
// a.mask_bits at the window's first vector; a.derived_group / a.row_alt as on the row-major routes
int launch_sweep_tiled(int P, int mode, const SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid) {
  if (a.prefix) {  // a.mv.data = the whole image, a.prefix_group = the counted group(s): enqueue_sweep filled them from the plan
    const uint32_t pvec = (uint32_t)(a.mv.pitch / 16);
    if (a.derived_group >= P || (a.derived_group >= 0 && !a.row_alt)) return fail(FMH_ERR_INVALID, "the tiled route takes a derived group with its row totals");
    // the epilogue of the table form works in 32 bits (site_const_epilogue.hpp): n^2 and n1 n2 below 2^32.  The table's own eligibility (u16 entries)
    // already implies it, so no plan reaches this refusal.
    if (a.mv.columns > kConstEpilogueMaxColumns) return fail(FMH_ERR_INVALID, "the table form of the tiled route takes at most %u columns", kConstEpilogueMaxColumns);
    for (int p = 0; p < P; ++p)
      if (a.group_size[p] > kConstEpilogueMaxColumns) return fail(FMH_ERR_INVALID, "the table form of the tiled route takes groups of at most %u columns", kConstEpilogueMaxColumns);
    for (int q = 0; q < P - (a.derived_group >= 0 ? 1 : 0); ++q) {
      const PrefixGroup& g = a.prefix_group[q];
      if (g.b_lo > g.b_hi || g.b_hi > pvec || g.n_edges > 2 || (g.n_edges > 0 && g.edge_vec[0] >= pvec) || (g.n_edges > 1 && g.edge_vec[1] >= pvec))
        return fail(FMH_ERR_INVALID, "a prefix-count group outside the row's %u vectors", pvec);
    }
#define ROW(PV, MODEV) if (P == PV && mode == (MODEV)) return launch_prefix_counted<PV, MODEV>(a, st, ctx, grid);
    FMH_TILED_BUILDS(ROW)
#undef ROW
    return fail(FMH_ERR_UNSUPPORTED, "no tiled sweep kernel for %d groups in mode %d", P, mode);
  }
  if (a.mv.nvec < 1 || a.mv.pitch < (size_t)a.mv.nvec * 16 || a.derived_group >= P || (a.derived_group >= 0 && !a.row_alt))
    return fail(FMH_ERR_INVALID, "the tiled route takes a window of 1..pitch / 16 vectors and a derived group with its row totals");
#define ROW(PV, MODEV) if (P == PV && mode == (MODEV)) return launch_counted<PV, MODEV>(a, st, ctx, grid);
  FMH_TILED_BUILDS(ROW)
#undef ROW
  return fail(FMH_ERR_UNSUPPORTED, "no tiled sweep kernel for %d groups in mode %d", P, mode);
}

}  // namespace fmhi
