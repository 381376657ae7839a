// sweep_plan.hpp — what ONE sweep does, decided once: the kernel group count, the column window, the launch route, the batch depth, the LDS a
// workgroup takes and the deferral's room, or the status and message of a combination that is refused.  plan_sweep() is a pure function of
// its arguments: it makes no HIP call, reads no option, no environment and no global (sweep_plan_check.hip runs it on a machine without a
// GPU and tests/sweep_plans.tsv holds what it must answer).  enqueue_sweep (sweep_dispatch.hip) fills the kernel arguments from the plan and
// dispatches on plan.route; the probes (fmh_sweep_window, fmh_sweep_tiled, fmh_sweep_prefix) and the helpers of the statistic entry points read the same plan
// or the predicates below, so that no caller re-derives a piece of the decision.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include "abi_internal.hpp"
#include "sweep_mfma_kernels.hpp"  // mfma_mask_stride

namespace fmhi {

// The switches a plan depends on, read once per enqueue (snapshot_plan_options, sweep_dispatch.hip).
struct PlanOptions {
  long long layout_bytes = 0, mask_mode = -1, defer_tiles = 0, packed_lpr = 0, packed_unroll = 0, packed_no_prefetch = 0, counts_mfma = 0, unroll = 0;
  long long flat = -1, wc_exact = 1, column_window = 1, tiled = -1, prefix_counts = 1;
};
// The device's two LDS figures (abi.hip): what a workgroup's masks may take, and the LDS of a CU.
struct LdsFigures {
  size_t limit, per_cu;
};

// ---- do the masks fit in LDS?  Two formulas, kept as they were: changing either changes routing ------------------------------------------
// (A) masks_lds_bits_bytes: the masks as BITS (the narrowest form a u8 sweep can keep in LDS), on the whole row padded to 64 vectors, for the
//     PADDED group count.  Asked BEFORE a sweep is planned, by the statistic entry points that must choose between one fused sweep and
//     several smaller ones: wc_fused_lane_totals, summaries_single_sweep, fmh_wc_sweep, fmh_population_summaries and fmh_wc_sweep_many's
//     batch sizes.  It is the layout-independent "does not fit in LDS in either form" test, so the answer is the same for the byte and the
//     packed image of one matrix and the callers' batching does not depend on FMH_LAYOUT.
// (B) masks_lds_bytes: what the planned kernel really takes - 16 bytes per mask vector, on the padded width of what it reads (the window on
//     packed rows, the row on u8 rows), for the KERNEL group count (five to seven exactly for W&C).  plan_sweep only: it sizes smem and picks
//     between the bytes / bits / global mask routes with it, and refuses a packed sweep that exceeds the limit.
// A packed vector holds 128 columns and a u8 vector 16, so on packed rows (B) is far inside (A)'s answer; on u8 rows (B) falling through to
// bits is (A)'s form.  Nothing requires the two to agree, and (A) failing always sends the caller to batches of two groups, which (B) takes
// at any width through the global-mask route.
inline size_t masks_lds_bits_bytes(int padded, size_t nvec) { return (size_t)padded * round_up(nvec, 64) * 2; }
inline size_t masks_lds_bytes(int P, uint32_t nvec_pad) { return (size_t)P * nvec_pad * 16; }
// the eight-group W&C kernels keep their regional sums through a static LDS scratch (sweep_kernels.hpp, wc_xpose_scratch): that much less for masks
inline size_t wc_lds_limit(size_t limit, int P) { return limit - (P >= 5 ? fmh::kWcXposeLdsBytes + 1024 : 0); }

// Which W&C / summaries calls are ONE fused sweep, by formula (A): wc_fused_lane_totals - fmh_wc_sweep runs one kernel that keeps the regional
// sums itself (2..8 groups, masks in LDS; registers up to four groups, the per-wave LDS transposition beyond), the route the pipelined sharded
// sweep can finalise and reduce on the device; everything else (alleles beyond 3 with five to eight groups, rows too wide for all masks) goes
// through the counts route - and summaries_single_sweep.
inline bool plan_wc_fused(const fmh_matrix& m, const fmh_groups& g, size_t limit) {
  if (g.padded == 8 && m.max_allele > 3) return false;
  return masks_lds_bits_bytes(g.padded, m.nvec) <= wc_lds_limit(limit, g.padded);
}
inline bool plan_summaries_single(const fmh_matrix& m, const fmh_groups& g, size_t limit) {
  return !(masks_lds_bits_bytes(g.padded, m.nvec) > limit && g.n_groups > 2);
}

enum class SweepRoute : int { none, tiled, flat, mfma, packed4, packed16, packed4_3p, packed16_3p, global, bits, bytes };

struct SweepPlan {
  int status = FMH_OK;  // FMH_OK, or the status of the refusal whose text is `message`
  char message[192] = {0};
  bool empty = false;   // the row range is empty: nothing is launched
  // the window and `tiled` are decided first and hold for every plan (the probes report them); the fields from `route` on are the launch's,
  // decided when status == FMH_OK and the range is not empty
  bool packed = false;  // the packed image is swept (FMH_LAYOUT=bytes keeps the byte kernels on matrices that still hold their bytes)
  int P = 0;            // the group count the kernel is instantiated with
  bool missing = false, general = false;
  ColumnWindow win{0, 0, -1};
  bool windowed = false;
  bool tiled = false;  // the sweep reads the tile-transposed image (decided with the window, before any refusal: the probes report both)
  // the table form of the tiled route (plan_prefix): every counted group is answered from the prefix counts; `win` stays the hull the groups
  // span (what fmh_sweep_window reports on every route), prefix_vecs is what the kernel still reads per row: the groups' edge vectors
  bool prefix = false;
  uint32_t prefix_vecs = 0;
  fmh::PrefixGroup prefix_group[2] = {};  // the counted groups in the kernel's order
  SweepRoute route = SweepRoute::none;
  int lpr = 16, unroll = 4;
  uint32_t nvec_pad = 0;
  bool single_trip = false;
  size_t smem = 0;
  bool defer = false;  // the kernel has the deferring tile loop: the three fields below are its arguments
  int defer_tiles = 0, defer_cap = 0;
  uint32_t defer_offset = 0;
};

// ---- the predicates of the plan, each evaluated once by plan_sweep -------------------------------------------------------------------------
inline bool plan_packed(const fmh_matrix& m, const PlanOptions& o) { return m.p0 && !(m.data && o.layout_bytes != 0); }

// The group count the W&C kernel of a sweep is instantiated with: the padded one (1, 2, 4, 8), or EXACTLY five, six or seven on a packed
// biallelic matrix with nothing missing - the slots of the padding are then not even compiled in (sweep_launch.inc).
inline int plan_wc_groups(const fmh_matrix& m, const fmh_groups& g, const PlanOptions& o) {
  if (g.n_groups >= 5 && g.n_groups <= 7 && plan_packed(m, o) && !m.has_missing && m.max_allele <= 1 && o.wc_exact != 0) return g.n_groups;
  return g.padded;
}

// Short packed rows, biallelic, nothing missing: the LDS-staged flat-tile route (sweep_flat_kernels.hpp: one row per lane, scalar masks).
// FMH_FLAT: 1 = wherever it is built, 0 = never, -1 = where it measured ahead of the four-lane route.  (Wanted is not taken: plan_sweep
// also asks for packed masks, no window and no matrix-core route.)
inline bool plan_flat_wanted(const fmh_matrix& m, const fmh_groups& g, int mode, bool packed, int P, const PlanOptions& o) {
  return packed && !m.has_missing && m.max_allele <= 1 && m.pvec <= (uint32_t)kFlatMaskMaxVec && g.mask_flat && flat_route_builds(P, mode) && o.flat != 0 &&
         (o.flat > 0 || flat_route_default(P, mode, m.pvec));
}

// Column window.  A vector in which no group has a member adds zero to every count, so a sweep reads only the hull of
// its groups' supports.  On a biallelic matrix with nothing missing the row's total alt count is a property of the resident image (row_alt), so
// when one or two groups PARTITION the columns one of them need not be counted: alt[g] = row_alt - alt[other], integers, the same bits.  The
// derived group is the one that leaves the shorter range to read (ties: the second group); nothing is derived when that saves no vector, e.g.
// interleaved membership.  At least one vector is always read (the kernels' loops have no zero-trip form).  The flat route stages whole rows.
inline ColumnWindow plan_window(const fmh_matrix& m, const fmh_groups& g, int mode, bool packed, bool flat_wanted, const PlanOptions& o) {
  ColumnWindow w{0, packed ? m.pvec : m.nvec, -1};
  if (!packed || m.max_allele > 1 || m.has_missing || m.p1 || m.pc || o.column_window == 0) return w;
  if (flat_wanted) return w;
  auto hull = [&](int skip, uint32_t* first, uint32_t* count) {
    uint32_t lo = UINT32_MAX, hi = 0;
    for (int p = 0; p < g.n_groups; ++p) {
      if (p == skip || g.vec_first[p] > g.vec_last[p]) continue;
      lo = std::min(lo, g.vec_first[p]);
      hi = std::max(hi, g.vec_last[p]);
    }
    if (lo == UINT32_MAX) { *first = 0; *count = 1; return; }  // no member anywhere: one vector, whose masks are zero
    *first = lo;
    *count = hi - lo + 1;
  };
  hull(-1, &w.first, &w.count);
  if ((mode & fmh::kModeWc) == 0 && g.n_groups <= 2 && m.row_alt && g.disjoint && g.covers) {
    for (int d = g.n_groups - 1; d >= 0; --d) {
      uint32_t first, count;
      hull(d, &first, &count);
      if (count < w.count) { w.first = first; w.count = count; w.derived = d; }
    }
  }
  return w;
}

// The tile-transposed image: a sweep of one or two groups over a packed biallelic matrix with nothing missing that holds
// the image can read its window from there - whole KiB per tile instead of pieces of 128-byte lines per row.  FMH_TILED: 1 = wherever the route
// is built, 0 = never, -1 = where it measured ahead of the row-major routes (tiled_route_default: a window of at most seven eighths of the
// row); never where the flat route is wanted.  The window itself is plan_window's, whichever route reads it.
inline bool plan_tiled(const fmh_matrix& m, const fmh_groups& g, int mode, bool packed, bool flat_wanted, const ColumnWindow& win, const PlanOptions& o) {
  if (!(packed && m.p0t && !m.has_missing && m.max_allele <= 1 && !m.p1 && !m.pc && o.tiled != 0 && (mode & fmh::kModeWc) == 0 && g.padded <= 2 &&
        g.n_groups == g.padded && tiled_route_builds(g.padded, mode) && !flat_wanted))
    return false;
  return o.tiled > 0 || tiled_route_default(win.count, m.pvec);
}

// One contiguous group [c0, c1) of a row of `pvec` vectors and `columns` columns as two table entries and at most two edge vectors.  Whole
// vectors: [ceil(c0 / 128), floor(c1 / 128)), and up to boundary pvec when the range ends with the row (P[pvec] is the row total: the last
// vector's columns past the row are not counted there).  What is left of the range on either side is an edge: part of one vector, read and
// counted under a mask.  A range inside one vector is that vector alone.
inline fmh::PrefixGroup plan_prefix_group(uint32_t c0, uint32_t c1, uint32_t pvec, uint32_t columns) {
  fmh::PrefixGroup g{};
  auto edge = [&](uint32_t lo, uint32_t hi) {  // columns [lo, hi) of one vector
    const uint32_t k = g.n_edges++, v = lo / 128;
    g.edge_vec[k] = v;
    for (uint32_t c = lo; c < hi; ++c) g.edge_mask[k][(c - v * 128) / 32] |= 1u << (c % 32);
  };
  const uint32_t v_lo = (c0 + 127) / 128, v_hi = c1 == columns ? pvec : c1 / 128;
  if (v_lo > v_hi) { edge(c0, c1); return g; }
  if (c0 % 128) edge(c0, std::min(v_lo * 128, c1));  // (a range that starts inside the row's last vector ends with the row, not the vector)
  if (v_hi < pvec && v_hi * 128 < c1) edge(v_hi * 128, c1);
  if (v_hi > v_lo) { g.b_lo = v_lo; g.b_hi = v_hi; }
  return g;
}

// The table form: on the tiled route of a matrix that holds the prefix counts, when EVERY counted group (all but the
// derived one) is one column range.  A sweep with a counted group that is not keeps today's window for all of its groups; one that counts
// nothing (a single group of every column) reads no vector either way.  FMH_PREFIX_COUNTS=0 keeps the window with the table present.
inline void plan_prefix(SweepPlan& p, const fmh_matrix& m, const fmh_groups& g, const PlanOptions& o) {
  if (!p.tiled || !m.p0c || o.prefix_counts == 0 || g.n_groups > 2) return;
  int n = 0;
  for (int i = 0; i < g.n_groups; ++i) {
    if (i == p.win.derived) continue;
    if (!g.contiguous[i] || g.col_end[i] > m.columns) return;
    p.prefix_group[n++] = plan_prefix_group(g.col_first[i], g.col_end[i], m.pvec, m.columns);
  }
  if (n == 0) return;
  p.prefix = true;
  for (int q = 0; q < n; ++q) p.prefix_vecs += p.prefix_group[q].n_edges;
}

__attribute__((format(printf, 3, 4))) inline const SweepPlan& plan_refuse(SweepPlan& p, int status, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p.message, sizeof p.message, fmt, ap);
  va_end(ap);
  p.status = status;
  return p;
}

inline SweepPlan plan_sweep(const fmh_matrix& m, const fmh_groups& g, int mode, size_t row_count, const PlanOptions& opt, const LdsFigures& lds) {
  using namespace fmh;
  SweepPlan p;
  const bool packed = p.packed = plan_packed(m, opt);
  const int P = p.P = mode == kModeWc ? plan_wc_groups(m, g, opt) : g.padded;
  const bool missing = p.missing = m.has_missing;
  const bool general = p.general = m.max_allele > 1;
  const bool flat_wanted = plan_flat_wanted(m, g, mode, packed, P, opt);
  p.win = plan_window(m, g, mode, packed, flat_wanted, opt);
  const uint32_t row_vecs = p.win.count;  // vectors a row of this sweep has: what sizes lanes per row, batch depth, LDS and deferral below
  p.windowed = packed && (p.win.first != 0 || p.win.count != m.pvec || p.win.derived >= 0);
  p.tiled = plan_tiled(m, g, mode, packed, flat_wanted, p.win, opt);
  plan_prefix(p, m, g, opt);
  if (row_count == 0) { p.empty = true; return p; }
  p.unroll = opt.unroll == 8 ? 8 : 4;
  p.nvec_pad = (uint32_t)round_up(m.nvec, 16 * p.unroll);
  size_t smem = masks_lds_bytes(P, p.nvec_pad);
  int mask_mode = kMaskLdsBytes;
  int lpr = 16;
  const size_t lds_limit = mode == kModeWc ? wc_lds_limit(lds.limit, P) : lds.limit;
  if (packed) {
    // 128 columns per vector.  Rows of up to 32 vectors (4 096 columns) are shared by FOUR lanes (no idle vector slots
    // on short rows, a two-step reduction: C2 0.081 -> 0.042 ms, C3 0.94 -> 0.63 ms), wider ones by the sixteen lanes of a
    // DPP row (C4's 40 vectors: 1.32 vs 1.34 ms, 200 000 columns: 0.46 vs 0.66 ms); the batch depth U (vectors per lane in
    // flight per trip) is the one with the fewest padded slots, ties to the deeper batch.  (Eight lanes per row measured between
    // the two everywhere - C4 1.37 ms - and is not built.  Round 3 built it once more for the narrow rows, where eight lanes read whole
    // 128-byte lines - 1 000 haplotypes: one contiguous KB per load instruction -: Hudson +4...+10 % at 1 000 haplotypes, +-1 % at 2 500; four-group
    // W&C +3...+18 %, summaries -1...+8 % (profiles/r03/ab_eight_lanes_per_row.jsonl).  The 64-byte segments of the four-lane rows are not what holds them back.)
    const int env_punroll = (int)opt.packed_unroll;
    const int env_lpr = (int)opt.packed_lpr;
    lpr = env_lpr == 4 || env_lpr == 16 ? env_lpr : (row_vecs <= 32 ? 4 : 16);
    // eight groups: the row loop of many batches is built with the shallow batches only (deeper ones kept P x U mask vectors and subset sums live and
    // spilled).  A biallelic row with nothing missing that ONE batch of loads per lane covers takes any depth: that loop (tile_rows_packed_prefetch,
    // MREG = false) re-reads its masks from LDS per row, and a 2 500-haplotype row is then one batch of five loads per lane instead of five trips
    // of one with a single vector in flight (five groups, which run the eight-group kernel: DESIGN.md section 3).
    const int us4[4] = {1, 2, 3, 5}, us16[3] = {2, 3, 4};
    const int* us = lpr != 16 ? us4 : us16;
    auto pick = [&](bool shallow) {
      const int nus = shallow ? (lpr != 16 ? 2 : 1) : (lpr != 16 ? 4 : 3);
      int best_u = us[0];
      size_t best = SIZE_MAX;
      for (int k = 0; k < nus; ++k) {
        const size_t slots = round_up(row_vecs, (size_t)lpr * us[k]);
        if (slots <= best) { best = slots; best_u = us[k]; }
      }
      p.unroll = best_u;
      for (int k = 0; k < nus; ++k) if (env_punroll == us[k]) p.unroll = env_punroll;
      p.nvec_pad = (uint32_t)round_up(row_vecs, (size_t)lpr * p.unroll);
    };
    const bool no_prefetch = opt.packed_no_prefetch != 0;
    pick(P >= 5 && (general || missing || no_prefetch));
    if (P >= 5 && p.nvec_pad != (uint32_t)(lpr * p.unroll)) pick(true);  // not one batch per row: the shallow set
    // The prefetching row loop (tile_rows_packed_prefetch) is taken when one batch of loads covers a row.  Same-process A/Bs (tools/ab_env.py
    // FMH_PACKED_NO_PREFETCH=1): on four-lane rows (1 000 and 2 500 haplotypes) it is level or 1-6 % ahead at every launch size; on sixteen-lane
    // rows with two groups (5 000 haplotypes) it was 2.4-2.9 % ahead at 625 k sites, level at 1 M and 0.6-2.4 % behind from 1.25 M to 10 M sites -
    // those kernels (one and two groups, sixteen lanes) have since dropped it altogether for the deferred-epilogue loop (sweep_kernel, defer_kernel()).
    p.single_trip = p.nvec_pad == (uint32_t)(lpr * p.unroll) && !no_prefetch;
    smem = masks_lds_bytes(P, p.nvec_pad);
    mask_mode = kMaskPacked;
    if (smem > lds_limit)
      return plan_refuse(p, FMH_ERR_UNSUPPORTED, "%d group masks of %u columns exceed the LDS budget: sweep fewer groups at a time on rows this wide", P, m.columns);
  } else if (smem > lds_limit) {  // byte masks do not fit LDS: bits in LDS if those fit, else bytes in global memory (L2)
    smem = (size_t)P * p.nvec_pad * 2;
    mask_mode = kMaskLdsBits;
    if (smem > lds_limit) { smem = 0; mask_mode = kMaskGlobalBytes; }
  }
  // BASELINE config C5: the counts as an int8 matrix-core contraction (sweep_mfma_kernels.hpp), for u8 rows that are biallelic with
  // nothing missing and at most four (padded) groups.  An alternative route: the contraction has <= 4 output rows and stays HBM-bound,
  // so it is measured beside the dot4 route, not chosen by default.
  const int env_mfma = (int)opt.counts_mfma;
  const int mfma_unroll = env_mfma == 2 ? 2 : 4;
  // (rows whose byte masks do not fit LDS stay on the dot4 routes)
  const bool fused_region = (mode & kModeDiversity) != 0 && P == 2;  // not built on the matrix-core route
  const bool mfma = !packed && !fused_region && env_mfma != 0 && !missing && !general && P <= 4 &&
                    masks_lds_bytes(P, mfma_mask_stride(m.nvec, mfma_unroll)) <= lds_limit;
  if (mfma) {
    p.unroll = mfma_unroll;
    p.nvec_pad = mfma_mask_stride(m.nvec, p.unroll);
    smem = masks_lds_bytes(P, p.nvec_pad);
  }
  const int want = packed || mfma ? -1 : (int)opt.mask_mode;
  if (want >= 0) {  // tests and measurements: take a slower mask route than needed
    const bool global_ok = P <= 2 && mode != kModeWc;
    if (want == kMaskLdsBits && mask_mode == kMaskLdsBytes) { smem = (size_t)P * p.nvec_pad * 2; mask_mode = kMaskLdsBits; }
    if (want == kMaskGlobalBytes && global_ok) { smem = 0; mask_mode = kMaskGlobalBytes; }
  }
  // Deferred epilogues (sweep_kernel, defer_kernel()): room behind the mask image for the counts a wave parks, as deep as leaves three workgroups
  // per CU their LDS (wide rows: the mask image takes it, and a tile of megabytes has nothing to gain from deferral anyway; measured: 200 000
  // columns fell from 3 to 2 workgroups per CU, 0.45 -> 0.69 ms, before the cap).  The deferring kernels have no other tile loop, so one tile's
  // room is always added.
  if (!mfma && defer_rule(P, mode, missing, general, lpr)) {  // the rule the kernel template is instantiated with
    const int e = (int)opt.defer_tiles;  // measurements (1 = the undeferred order); default -1 = by the launch size (launch_one)
    p.defer = true;
    p.defer_tiles = e >= 1 && e <= kDeferTiles ? e : -1;
    smem = round_up(smem, 16);
    int depth = defer_depth_host(P, mode, missing);
    while (depth > 1 && smem + defer_lds_bytes(P, mode, missing, depth) > lds.per_cu / 3 - 1024) depth /= 2;
    p.defer_cap = depth;
    p.defer_offset = (uint32_t)smem;
    smem += defer_lds_bytes(P, mode, missing, depth);
  }
  p.lpr = lpr;
  p.smem = smem;
  // argument checks shared by every route
  if (mode == (kModeSummary | kModeHudson) && P != 2) return plan_refuse(p, FMH_ERR_INVALID, "Hudson sweep needs exactly 2 groups");
  if (mode == (kModeSummary | kModeDiversity) && P > 2) return plan_refuse(p, FMH_ERR_INVALID, "diversity sweep needs 1 group (or the 2 of a fused region sweep)");
  if (mode == (kModeSummary | kModeHudson | kModeDiversity) && P != 2) return plan_refuse(p, FMH_ERR_INVALID, "the fused region sweep needs exactly 2 groups");
  if (mode == kModeWc && P == 1) return plan_refuse(p, FMH_ERR_INVALID, "W&C sweep needs at least 2 groups");
  if (mode != kModeSummary && mode != (kModeSummary | kModeHudson) && mode != (kModeSummary | kModeDiversity) && mode != (kModeSummary | kModeHudson | kModeDiversity) &&
      mode != kModeWc)
    return plan_refuse(p, FMH_ERR_UNSUPPORTED, "unsupported sweep mode %d", mode);
  if (mask_mode == kMaskGlobalBytes && (P > 2 || mode == kModeWc))
    return plan_refuse(p, FMH_ERR_UNSUPPORTED, "%d group masks of %u columns exceed the LDS budget: sweep at most two groups at a time on rows this wide", P, m.columns);
  const bool flat = mask_mode == kMaskPacked && !p.windowed && !mfma && flat_wanted;
  if (p.tiled) p.route = SweepRoute::tiled;
  else if (flat) p.route = SweepRoute::flat;
  else if (mfma) p.route = SweepRoute::mfma;
  else if (mask_mode == kMaskPacked && general && m.p2) p.route = lpr == 4 ? SweepRoute::packed4_3p : SweepRoute::packed16_3p;  // alleles 4..7: three planes
  else if (mask_mode == kMaskPacked) p.route = lpr == 4 ? SweepRoute::packed4 : SweepRoute::packed16;
  else if (mask_mode == kMaskGlobalBytes) p.route = SweepRoute::global;
  else if (mask_mode == kMaskLdsBits) p.route = SweepRoute::bits;
  else p.route = SweepRoute::bytes;
  return p;
}

}  // namespace fmhi
