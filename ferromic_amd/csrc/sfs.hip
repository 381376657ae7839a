// sfs.hip — site frequency spectra: fmh_sfs (the 1-D spectrum of one group per row window), fmh_sfs_joint (the joint spectrum of two
// groups) and fmh_sfs_stats (S, pi, theta_W, theta_H, Tajima's D and Fay & Wu's H of one spectrum, host only).  Kernel in
// sfs_kernels.hpp; definition in include/ferromic_hip.h, the item / LDS tile / corner scheme in DESIGN.md section 3.12.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "abi_internal.hpp"
#include "sfs_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

constexpr size_t kSfsMaxBins = (size_t)1 << 28;          // bins of one call's table
constexpr size_t kSfsDefaultItemRows = 4096;             // measured ahead of 1 024 and 16 384 at 10 M rows
// the largest tile ONE 512-thread workgroup per CU can hold beside the kernel's head: eight waves resident at any n
constexpr size_t kSfsMaxLdsBins = kLdsPerCu / 4 - kSfsLdsHead;
// the default cap: the largest tile that still lets EIGHT 256-thread workgroups share a CU (a joint spectrum measured 2x faster at that
// occupancy than with one 512-thread workgroup and a 160 KiB tile); a 1-D spectrum of 5 000 haplotypes fits whole
constexpr size_t kSfsDefaultLdsBins = kLdsPerCu / 8 / 4 - kSfsLdsHead;

// every refusal that needs no device, in the header's order; *bins = one window's slice
int check_args(const fmh_matrix* m, const fmh_groups* g, int want_groups, const void* d_sfs, const RowSpan* windows, size_t n_windows,
               bool windows_given, size_t* bins) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!g) return fail(FMH_ERR_INVALID, "NULL groups");
  if (!d_sfs) return fail(FMH_ERR_INVALID, "d_sfs is NULL");
  if (!windows_given) return fail(FMH_ERR_INVALID, "h_windows is NULL");
  if (g->n_groups != want_groups)
    return fail(FMH_ERR_INVALID, "%s takes exactly %d group%s, got %d", want_groups == 1 ? "the site frequency spectrum" : "the joint site frequency spectrum",
                want_groups, want_groups == 1 ? "" : "s", g->n_groups);
  if (g->device != m->device || g->columns != m->columns) return fail(FMH_ERR_INVALID, "the groups were not made for this matrix");
  for (int p = 0; p < want_groups; ++p)
    if (g->sizes[p] == 0) return fail(FMH_ERR_INVALID, "group %d has no member", p);
  FMH_TRY(check_row_spans(windows, n_windows, "window", m->variants));
  if (n_windows == 0) return fail(FMH_ERR_INVALID, "n_windows is 0");
  size_t slice = (size_t)g->sizes[0] + 1;
  if (want_groups == 2) slice *= (size_t)g->sizes[1] + 1;  // both factors are below 2^32
  if (slice > kSfsMaxBins || n_windows > kSfsMaxBins / slice)
    return fail(FMH_ERR_UNSUPPORTED, "a table of %zu windows x %zu bins exceeds 2^28 bins", n_windows, slice);
  FMH_TRY(check_packed(m, "the site frequency spectrum reads"));
  *bins = slice;
  return FMH_OK;
}

// the on-chip tile of a call: which keys of each axis stay in LDS under a budget of `budget` bins (at least 4)
void plan_tile(size_t budget, uint32_t n0, uint32_t n1, bool joint, SfsAxis* ax0, SfsAxis* ax1) {
  auto whole = [](uint32_t n) { return SfsAxis{n, n + 1, n + 1}; };
  auto ends = [](uint32_t n, size_t slots) { const uint32_t T = (uint32_t)(slots / 2); return SfsAxis{n, T, 2 * T}; };
  if (!joint) {
    *ax0 = (size_t)n0 + 1 <= budget ? whole(n0) : ends(n0, budget);
    *ax1 = SfsAxis{0, 1, 1};
    return;
  }
  // corners: 4 T0 T1 bins.  Start from a square, then hand what a short axis leaves to the other one.
  size_t side = 2;
  while ((side + 2) * (side + 2) <= budget) side += 2;
  size_t l0 = std::min<size_t>((size_t)n0 + 1, side);
  size_t l1 = std::min<size_t>((size_t)n1 + 1, std::max<size_t>(budget / l0, 2));
  l0 = std::min<size_t>((size_t)n0 + 1, std::max<size_t>(budget / l1, 2));
  *ax0 = l0 == (size_t)n0 + 1 ? whole(n0) : ends(n0, l0);
  *ax1 = l1 == (size_t)n1 + 1 ? whole(n1) : ends(n1, l1);
}

int run(const fmh_matrix* m, const fmh_groups* g, bool joint, const RowSpan* windows, size_t n_windows, size_t bins, uint64_t* d_sfs,
        fmh_sfs_skipped* h_skipped, void* stream) {
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  HIP_TRY(hipMemsetAsync(d_sfs, 0, n_windows * bins * sizeof(uint64_t), st));
  if (h_skipped) memset(h_skipped, 0, n_windows * sizeof(fmh_sfs_skipped));

  // work items: at most item_rows rows each, never across a window
  const size_t item_rows = item_rows_of(options().sfs_item_rows, kSfsDefaultItemRows);
  std::vector<SfsItem> items;
  for (size_t w = 0; w < n_windows; ++w)
    for (size_t r = windows[w].begin; r < windows[w].end; r += item_rows) {
      FMH_TRY(check_item_count(items.size() + 1, "FMH_SFS_ITEM_ROWS"));
      items.push_back(SfsItem{(unsigned long long)r, (uint32_t)std::min(item_rows, windows[w].end - r), (uint32_t)w});
    }
  if (items.empty()) {
    HIP_TRY(hipStreamSynchronize(st));
    return FMH_OK;
  }

  SfsArgs a{};
  set_plane_rows(a, m);
  const uint8_t* mask_bits = reinterpret_cast<const uint8_t*>(g->mask_bits);  // one bit per column, a group's row is mask_pitch / 8 bytes
  a.mask0 = mask_bits;
  a.mask1 = joint ? mask_bits + g->mask_pitch / 8 : mask_bits;
  a.vec_begin = g->vec_first[0];
  a.vec_end = g->vec_last[0] + 1;
  if (joint) {
    a.vec_begin = std::min(a.vec_begin, g->vec_first[1]);
    a.vec_end = std::max(a.vec_end, g->vec_last[1] + 1);
  }
  a.vec_end = std::min(a.vec_end, m->pvec);

  // LDS: dynamic, sized by the tile the call needs.  Up to half of a CU's LDS per workgroup: 256 threads, two or more workgroups per CU;
  // beyond that one 512-thread workgroup per CU - eight waves per CU either way.
  int lds_max = 0;
  HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, m->device));
  const size_t lds_cap = std::min<size_t>(kLdsPerCu, (size_t)std::max(lds_max, 1024));
  long long opt_bins = options().sfs_lds_bins.load(std::memory_order_relaxed);
  size_t budget = opt_bins <= 0 ? kSfsDefaultLdsBins : (size_t)std::min<long long>(opt_bins, (long long)kSfsMaxLdsBins);
  budget = std::max<size_t>(std::min(budget, lds_cap / 4 - kSfsLdsHead), 4);
  plan_tile(budget, (uint32_t)g->sizes[0], joint ? (uint32_t)g->sizes[1] : 0, joint, &a.ax0, &a.ax1);
  const size_t lds_bytes = ((size_t)a.ax0.L * a.ax1.L + kSfsLdsHead) * sizeof(uint32_t);
  const bool wide = lds_bytes > kLdsPerCu / 2;
  const unsigned threads = wide ? 512 : 256;
  const size_t per_cu = wide ? 1 : std::min<size_t>(8, kLdsPerCu / lds_bytes);
  const unsigned grid = (unsigned)std::min<size_t>(items.size(), (size_t)std::max(call.ws->cus, 1) * per_cu);

  SfsItem* d_items = nullptr;
  FMH_TRY(call.upload(items.data(), items.size(), &d_items));
  unsigned long long* d_skipped = nullptr;
  if (h_skipped) FMH_TRY(call.zeroed(n_windows * 2, &d_skipped));
  a.items = d_items;
  a.n_items = (uint32_t)items.size();
  a.bins = bins;
  a.sfs = reinterpret_cast<unsigned long long*>(d_sfs);
  a.skipped = d_skipped;

  // four lanes per row while a row's window is at most four vectors (one 16-byte load per lane covers it), sixteen beyond
  const bool lanes4 = a.vec_end - a.vec_begin <= 4;
  void (*kernel)(const SfsArgs) = joint ? (lanes4 ? sfs_kernel<4, true> : sfs_kernel<16, true>) : (lanes4 ? sfs_kernel<4, false> : sfs_kernel<16, false>);
  if (lds_bytes > ((size_t)64 << 10))
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));

  FMH_TRY(call.start());
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  FMH_TRY(call.stop());
  static_assert(sizeof(fmh_sfs_skipped) == 2 * sizeof(unsigned long long), "fmh_sfs_skipped is two u64");
  if (h_skipped) HIP_TRY(hipMemcpyAsync(h_skipped, d_skipped, n_windows * sizeof(fmh_sfs_skipped), hipMemcpyDeviceToHost, st));
  return call.finish();
}

}  // namespace

extern "C" int fmh_sfs(const fmh_matrix* m, const fmh_groups* g, const uint64_t* h_windows, size_t n_windows, uint64_t* d_sfs,
                       fmh_sfs_skipped* h_skipped_or_null, void* stream) {
  const RowSpan* windows = reinterpret_cast<const RowSpan*>(h_windows);
  size_t bins = 0;
  FMH_TRY(check_args(m, g, 1, d_sfs, windows, n_windows, h_windows != nullptr, &bins));
  return run(m, g, false, windows, n_windows, bins, d_sfs, h_skipped_or_null, stream);
}

extern "C" int fmh_sfs_joint(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, uint64_t* d_sfs,
                             fmh_sfs_skipped* h_skipped_or_null, void* stream) {
  // (a range whose end wraps is outside every matrix)
  const RowSpan window{row_begin, row_count <= std::numeric_limits<size_t>::max() - row_begin ? row_begin + row_count : std::numeric_limits<size_t>::max()};
  size_t bins = 0;
  FMH_TRY(check_args(m, g, 2, d_sfs, &window, 1, true, &bins));
  return run(m, g, true, &window, 1, bins, d_sfs, h_skipped_or_null, stream);
}

extern "C" int fmh_sfs_stats(const uint64_t* h_sfs, size_t n, fmh_sfs_stats_out* h_out) {
  if (!h_sfs || !h_out) return fail(FMH_ERR_INVALID, "NULL argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  fmh_sfs_stats_out o{};
  for (size_t k = 0; k <= n; ++k) o.sites += h_sfs[k];
  for (size_t k = 1; k < n; ++k) o.segregating_sites += h_sfs[k];
  o.pi_sum = o.theta_w_sum = o.theta_h_sum = o.tajima_d = o.fay_wu_h = nan;
  if (n >= 2) {
    // every term is non-negative; 2 k (n - k) and 2 k^2 are exact integers, the common divisor n (n - 1) is applied once
    const double nd = (double)n, pairs = nd * (nd - 1.0);
    double pi = 0.0, th = 0.0, a1 = 0.0, a2 = 0.0;
    for (size_t k = 1; k < n; ++k) {
      const double c = (double)h_sfs[k], kd = (double)k;
      pi += c * (2.0 * kd * (double)(n - k));
      th += c * (2.0 * kd * kd);
      a1 += 1.0 / kd;
      a2 += 1.0 / (kd * kd);
    }
    const double S = (double)o.segregating_sites;
    o.pi_sum = pi / pairs;
    o.theta_h_sum = th / pairs;
    o.theta_w_sum = S / a1;
    o.fay_wu_h = o.pi_sum - o.theta_h_sum;
    if (o.segregating_sites != 0 && n >= 4) {
      const double b1 = (nd + 1.0) / (3.0 * (nd - 1.0));
      const double b2 = 2.0 * (nd * nd + nd + 3.0) / (9.0 * nd * (nd - 1.0));
      const double c1 = b1 - 1.0 / a1;
      const double c2 = b2 - (nd + 2.0) / (a1 * nd) + a2 / (a1 * a1);
      const double e1 = c1 / a1, e2 = c2 / (a1 * a1 + a2);
      o.tajima_d = (o.pi_sum - o.theta_w_sum) / std::sqrt(e1 * S + e2 * S * (S - 1.0));
    }
  }
  *h_out = o;
  return FMH_OK;
}
