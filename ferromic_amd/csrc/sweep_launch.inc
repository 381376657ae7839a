// sweep_launch.inc — the instantiations of fmh::sweep_kernel for ONE mask route, and their launcher.  Included by
// sweep_packed4.hip, sweep_packed16.hip, sweep_bytes.hip, sweep_bits.hip and sweep_global.hip with
//   FMH_ROUTE_FN   name of the exported launcher (declared in abi_internal.hpp)
//   FMH_ROUTE_MM   kMaskPacked / kMaskLdsBytes / kMaskLdsBits / kMaskGlobalBytes
//   FMH_ROUTE_LPR  lanes per row (4 or 16)
//   FMH_ROUTE_NPL  (optional) 3: ONLY the multi-allelic kernels of a three-plane packed matrix (alleles 4..7)
// defined, so that the routes compile in parallel and a host-side edit of abi.hip does not rebuild any kernel.
#include "abi_internal.hpp"
#include "sweep_grid.hpp"

using namespace fmh;

#ifndef FMH_ROUTE_NPL
#define FMH_ROUTE_NPL 2
#endif

namespace fmhi {
namespace {

template <int P, int MODE, bool MISSING, bool GENERAL, int MM, int LPR, bool PIPE = false>
int launch_one(const SweepArgs& args, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid_out) {
  // the pipelined tile loop (sweep_kernel_pipe): four-lane packed rows, biallelic, nothing missing, one batch of loads per row
  constexpr bool kPipeBuilt = MM == kMaskPacked && LPR == 4 && !MISSING && !GENERAL && P <= 4;  // (one, two and four groups)
  // Same-process A/Bs over three boxes (profiles/r03/pipelined_tile_loop.jsonl): Hudson sweeps of 1 000 haplotypes -3 % at 10 M sites, -7 ... -9 % at
  // 1 M and below (C2: 0.0404 -> 0.0375 ms), 2 500 haplotypes -1 ... -2 %; four-group summaries -1 ... -2 % on long launches, +2.5 % on the
  // shortest; four-group W&C +-1 %.  Default: one and two groups.  (FOUR row steps of loads in flight instead of two - the whole next tile -: Hudson +1...+2 % at
  // 1 000 haplotypes, +4...+15 % at 2 500; four-group summaries -2...-5 % on some launches, +6...+9 % on others; W&C +0...+10 %, profiles/r03/
  // ab_pipelined_loop_four_steps_in_flight.jsonl: the loads a wave has in flight are not what limits these kernels.)
  if constexpr (kPipeBuilt && !PIPE) {
    const long long want = options().pipe.load();
    if (args.single_trip && (want == 1 || (want < 0 && P <= 2))) return launch_one<P, MODE, MISSING, GENERAL, MM, LPR, true>(args, smem, st, ctx, grid_out);
  }
  void (*kern)(const SweepArgs);
  if constexpr (PIPE) kern = sweep_kernel_pipe<P, MODE, LPR>;
  else kern = sweep_kernel<P, MODE, MISSING, GENERAL, MM, LPR, GENERAL ? FMH_ROUTE_NPL : 2>;
  static thread_local OccupancyCache cache;  // keyed by the dynamic LDS
  if (smem > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  // sixteen-lane packed rows: three workgroups per CU whatever the occupancy allows - round 2 measured 2, 4, 6 and 8 per CU 14-22 % / 17-22 % /
  // 0-5 % / 1.5-6 % behind 3 on the C4 sweep, and the one-instruction popcount chain left these kernels at 93-119 VGPRs (4-5 waves per SIMD)
  constexpr int kCeiling = MM == kMaskPacked && LPR == 16 && !GENERAL ? 3 : 8;
  int occ = 0;
  FMH_TRY(cached_occupancy(kern, kBlock, smem, kCeiling, false, cache, smem, &occ));
  const size_t ntiles = (args.row_count + kTileRows - 1) / kTileRows;
  const size_t blocks = persistent_grid(occ, args.row_count, kWavesPerBlock, ctx);
  SweepArgs launch_args = args;
  if (launch_args.defer_tiles < 0) {
    // Deferred epilogues (sweep_kernel, kDefer): how many of its tiles a wave counts before it runs their epilogues, by the tiles it sweeps in
    // all ("rounds") and the bytes a tile reads.  Same-process A/Bs (tools/ab_env.py FMH_DEFER_TILES=n; 1 = undeferred):
    //   5 000 haplotypes (40 KB per tile), against 16: 51 rounds 1 +9.2 %, 2 +2.9 %, 4 +7.6 %, 8 +2.4 %, 12 +0.1 %; 25 rounds 1 +8.0 %, 2 +0.5 %,
    //     12 -1.1 %; 13 rounds 2 and 8 level, 1 +3.6 %; 6 rounds 2 best (1 +4.6 %, 8 +3 %);
    //   the same with 1 % missing calls (80 KB per tile, 8 tiles deep at most): 25 rounds 1 +9.5 %; 13 rounds 8 best (2 +7 %, 1 +10 %); 6 and 3
    //     rounds 8 best by 2-3 %;
    //   four-lane rows (before those kernels went back to the plain tile loop, defer_kernel()): 2 500 haplotypes (20 KB) 25 rounds 8-12 best
    //     (1 +7 %), 13 rounds 8 best, 6 rounds 2; 1 000 haplotypes (8 KB): level or 2 % worse with any deferral at 3 to 51 rounds;
    //   (A second box agreed on the 40-KB rows (+11.6 / +10.5 / +8.0 / +3.4 % undeferred at 51 / 25 / 13 / 6 rounds) and showed smaller gains
    //   elsewhere: 20-KB rows +2.6 % at 25 rounds and a depth of 2 on short launches 2-4 % BEHIND 1, hence 1 there.)
    const size_t rounds = (ntiles + blocks * kWavesPerBlock - 1) / (blocks * kWavesPerBlock);
    const size_t tile_bytes = (size_t)kTileRows * args.mv.pitch * (MISSING ? 2 : 1);
    int ch;
    if (tile_bytes < (16u << 10)) ch = 1;
    else if (rounds >= 32) ch = kDeferTiles;
    else if (rounds >= 16) ch = 12;
    else if (rounds >= (tile_bytes >= (64u << 10) ? 3u : 8u)) ch = 8;
    else ch = tile_bytes >= (32u << 10) ? 2 : 1;
    launch_args.defer_tiles = ch;
  }
  return timed_launch(kern, blocks, kBlock, smem, st, ctx, launch_args, grid_out);
}

template <int P, int MODE>
int launch_pm(const SweepArgs& a, size_t smem, hipStream_t st, bool missing, bool general, const LaunchCtx& ctx, int* grid) {
  constexpr int MM = FMH_ROUTE_MM, LPR = FMH_ROUTE_LPR;
#if FMH_ROUTE_NPL == 3
  if (!general) return fail(FMH_ERR_UNSUPPORTED, "the three-plane launcher holds the multi-allelic kernels only");
  return missing ? launch_one<P, MODE, true, true, MM, LPR>(a, smem, st, ctx, grid) : launch_one<P, MODE, false, true, MM, LPR>(a, smem, st, ctx, grid);
#else
  if (missing) return general ? launch_one<P, MODE, true, true, MM, LPR>(a, smem, st, ctx, grid) : launch_one<P, MODE, true, false, MM, LPR>(a, smem, st, ctx, grid);
  return general ? launch_one<P, MODE, false, true, MM, LPR>(a, smem, st, ctx, grid) : launch_one<P, MODE, false, false, MM, LPR>(a, smem, st, ctx, grid);
#endif
}

}  // namespace

int FMH_ROUTE_FN(int P, int mode, bool missing, bool general, const SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid) {
#define CASE(PV, MODEV) return launch_pm<PV, MODEV>(a, smem, st, missing, general, ctx, grid)
  if (mode == kModeSummary) {
    if (P == 1) CASE(1, kModeSummary);
    if (P == 2) CASE(2, kModeSummary);
#if FMH_ROUTE_MM != 1  // the global-mask route sweeps one or two groups at a time (callers re-batch)
    if (P == 4) CASE(4, kModeSummary);
    if (P == 8) CASE(8, kModeSummary);
#endif
  } else if (mode == (kModeSummary | kModeHudson)) {
    if (P == 2) CASE(2, kModeSummary | kModeHudson);
  } else if (mode == (kModeSummary | kModeDiversity)) {
    if (P == 1) CASE(1, kModeSummary | kModeDiversity);
    if (P == 2) CASE(2, kModeSummary | kModeDiversity);  // fused region sweep without a Hudson part: summaries + per-site diversity of both groups
  } else if (mode == (kModeSummary | kModeHudson | kModeDiversity)) {
    if (P == 2) CASE(2, kModeSummary | kModeHudson | kModeDiversity);  // fused region sweep (fmh_pair_region_sweep)
  }
#if FMH_ROUTE_MM != 1
  else if (mode == kModeWc) {
    if (P == 2) CASE(2, kModeWc);
    if (P == 4) CASE(4, kModeWc);
#if FMH_ROUTE_NPL != 3  // eight groups with alleles beyond 3 go through the counts route (fmh_wc_sweep)
    if (P == 8) CASE(8, kModeWc);
#if FMH_ROUTE_MM == 3
    // five, six and seven groups EXACTLY (round 4; enqueue_sweep's wc_kernel_groups): biallelic packed matrices with nothing missing.  As the padded
    // eight-group kernel a five-group site computed, stored-or-skipped and summed 29 slots of which 11 exist (0.34 ms at 2 M x 2 500, the
    // 1000 Genomes super-population case); here the slot loops end at the caller's group count at compile time.
    if (P >= 5 && P <= 7) {
      if (missing || general) return fail(FMH_ERR_UNSUPPORTED, "the exact five-to-seven-group W&C kernels take biallelic matrices with nothing missing");
      if (P == 5) return launch_one<5, kModeWc, false, false, FMH_ROUTE_MM, FMH_ROUTE_LPR>(a, smem, st, ctx, grid);
      if (P == 6) return launch_one<6, kModeWc, false, false, FMH_ROUTE_MM, FMH_ROUTE_LPR>(a, smem, st, ctx, grid);
      return launch_one<7, kModeWc, false, false, FMH_ROUTE_MM, FMH_ROUTE_LPR>(a, smem, st, ctx, grid);
    }
#endif
#endif
  }
#endif
#undef CASE
  return fail(FMH_ERR_UNSUPPORTED, "no sweep kernel for %d groups in mode %d on this mask route", P, mode);
}

}  // namespace fmhi
