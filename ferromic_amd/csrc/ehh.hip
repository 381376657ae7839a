// ehh.hip — extended haplotype homozygosity scans: fmh_ehh_scan (per focal row and side the integers behind iHS and nSL: pair counts of the
// two core classes folded by the stop rules), fmh_ehh_stats (iHH, SL, iHS and nSL of the records, host only) and fmh_ehh_max_members.
// Kernel in ehh_kernels.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.14.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "abi_internal.hpp"
#include "ehh_kernels.hpp"
#include "hap_launch.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

static_assert(sizeof(fmh_ehh_side) == 56 && sizeof(EhhSide) == sizeof(fmh_ehh_side), "fmh_ehh_side is 56 bytes");
static_assert(FMH_EHH_EDGE0 == kEhhEdge0 && FMH_EHH_EDGE1 == 2 * kEhhEdge0 && FMH_EHH_GAP0 == kEhhGap0 && FMH_EHH_GAP1 == 2 * kEhhGap0 &&
                  FMH_EHH_SKIPPED == kEhhSkipped, "the kernel's flags are the header's");

namespace {

// every refusal, in the header's order; none needs a device
int check_args(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_end, const uint64_t* focal, size_t n_focal,
               const uint32_t* positions, const fmh_ehh_params* p, const void* d_out, bool want_pairs) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!g) return fail(FMH_ERR_INVALID, "NULL groups");
  if (!focal) return fail(FMH_ERR_INVALID, "h_focal is NULL");
  if (!p) return fail(FMH_ERR_INVALID, "params is NULL");
  if (!d_out) return fail(FMH_ERR_INVALID, "d_out is NULL");
  if (g->n_groups != 1) return fail(FMH_ERR_INVALID, "the haplotype scan takes exactly 1 group, got %d", g->n_groups);
  if (g->device != m->device || g->columns != m->columns) return fail(FMH_ERR_INVALID, "the groups were not made for this matrix");
  if (g->sizes[0] == 0) return fail(FMH_ERR_INVALID, "group 0 has no member");
  FMH_TRY(check_rows(row_begin, row_end - row_begin, m->variants));  // (row_end below row_begin wraps to a count no matrix holds)
  for (size_t i = 0; i < n_focal; ++i)
    if (focal[i] < row_begin || focal[i] >= row_end)
      return fail(FMH_ERR_INVALID, "focal row %llu (entry %zu) is outside the rows [%zu, %zu)", (unsigned long long)focal[i], i, row_begin, row_end);
  if (n_focal == 0) return fail(FMH_ERR_INVALID, "n_focal is 0");
  if (p->min_ehh_den == 0) return fail(FMH_ERR_INVALID, "min_ehh_den is 0");
  if (p->min_ehh_num > p->min_ehh_den) return fail(FMH_ERR_INVALID, "min_ehh_num %u exceeds min_ehh_den %u", p->min_ehh_num, p->min_ehh_den);
  if (positions)
    for (size_t r = row_begin + 1; r < row_end; ++r)
      if (positions[r] < positions[r - 1])
        return fail(FMH_ERR_INVALID, "the positions descend at row %zu (%u after %u)", r, positions[r], positions[r - 1]);
  if (want_pairs && p->max_extent == 0) return fail(FMH_ERR_INVALID, "d_pairs needs a max_extent (it is 0 = unlimited)");
  if (g->sizes[0] > kEhhMaxMembers)
    return fail(FMH_ERR_UNSUPPORTED, "a group of %llu members exceeds the %u the haplotype scan holds on chip (fmh_ehh_max_members)",
                (unsigned long long)g->sizes[0], kEhhMaxMembers);
  if (want_pairs && n_focal > ((size_t)1 << 32) / 4 / (size_t)p->max_extent)
    return fail(FMH_ERR_UNSUPPORTED, "a curve table of %zu focal rows x 2 sides x 2 cores x %u steps exceeds 2^32 entries", n_focal, p->max_extent);
  return check_packed(m, "the haplotype scan reads");
}

}  // namespace

extern "C" uint32_t fmh_ehh_max_members(void) { return kEhhMaxMembers; }

extern "C" int fmh_ehh_scan(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_end, const uint64_t* h_focal, size_t n_focal,
                            const uint32_t* h_positions_or_null, const fmh_ehh_params* params, fmh_ehh_side* d_out, uint32_t* d_pairs_or_null,
                            void* stream) {
  FMH_TRY(check_args(m, g, row_begin, row_end, h_focal, n_focal, h_positions_or_null, params, d_out, d_pairs_or_null != nullptr));
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));

  // the members' columns, ascending: member rank -> column
  const uint32_t n = (uint32_t)g->sizes[0];
  std::vector<uint32_t> cols;
  cols.reserve(n);
  for (uint32_t c = 0; c < g->columns; ++c)
    if (g->host_mask[c]) cols.push_back(c);
  if (cols.size() != n) return fail(FMH_ERR_INVALID, "the group's mask and size disagree");

  const size_t lds_bytes = hap_lds_bytes(n);
  int lds_max = 0;
  HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, m->device));
  if (lds_bytes > (size_t)std::max(lds_max, 0))
    return fail(FMH_ERR_UNSUPPORTED, "a group of %u members needs %zu bytes of LDS, this device gives a workgroup %d", n, lds_bytes, lds_max);

  const size_t n_items = n_focal * 2;
  const unsigned threads = hap_pick_threads(n, n_items, call.ws->cus);

  uint32_t* d_cols = nullptr;
  unsigned long long* d_focal = nullptr;
  uint32_t* d_pos = nullptr;
  FMH_TRY(call.upload(cols.data(), cols.size(), &d_cols));
  FMH_TRY(call.upload(h_focal, n_focal, &d_focal));
  if (h_positions_or_null) FMH_TRY(call.upload(h_positions_or_null + row_begin, row_end - row_begin, &d_pos));  // the rows of the range only

  EhhArgs a{};
  set_plane_rows(a, m);
  a.cols = d_cols;
  a.n = n;
  a.touch_first = (cols.front() >> 5) * 4;
  a.touch_last = (cols.back() >> 5) * 4;
  a.focal = d_focal;
  a.n_items = n_items;
  a.row_begin = row_begin;
  a.row_end = row_end;
  a.pos = d_pos;
  a.num = params->min_ehh_num; a.den = params->min_ehh_den;
  a.max_extent = params->max_extent; a.max_gap = params->max_gap; a.min_core = params->min_core;
  a.out = reinterpret_cast<EhhSide*>(d_out);
  a.pairs = d_pairs_or_null;

  const int planes = m->p2 ? 3 : m->p1 ? 2 : 1;
  void (*kernel)(const EhhArgs) = m->pc ? (planes == 3 ? ehh_kernel<3, true> : planes == 2 ? ehh_kernel<2, true> : ehh_kernel<1, true>)
                                        : (planes == 3 ? ehh_kernel<3, false> : planes == 2 ? ehh_kernel<2, false> : ehh_kernel<1, false>);
  if (lds_bytes > ((size_t)64 << 10))
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  // launch shape (hap_launch.hpp, stat_call.hpp), with the kernel's registers in it: at 81-88 VGPRs five waves fit a SIMD, fewer workgroups than LDS allows
  size_t grid = 0;
  FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), threads, lds_bytes, n_items, call.ws->cus, &grid));

  FMH_TRY(call.start());
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds_bytes, call.st, a);
  HIP_TRY(hipGetLastError());
  return call.finish();
}

extern "C" int fmh_ehh_stats(const fmh_ehh_side* h_sides, size_t n_focal, int include_edges, fmh_ehh_stats_out* h_out) {
  if (!h_sides || !h_out) return fail(FMH_ERR_INVALID, "NULL argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < n_focal; ++i) {
    const fmh_ehh_side &L = h_sides[2 * i], &R = h_sides[2 * i + 1];
    if (L.core[0] != R.core[0] || L.core[1] != R.core[1] || ((L.flags ^ R.flags) & FMH_EHH_SKIPPED))
      return fail(FMH_ERR_INVALID, "the two records of focal %zu are not of one focal row", i);
    fmh_ehh_stats_out& o = h_out[i];
    const uint32_t flags = L.flags | R.flags;
    const bool usable = !(flags & FMH_EHH_SKIPPED) && (include_edges || !(flags & (FMH_EHH_EDGE0 | FMH_EHH_EDGE1 | FMH_EHH_GAP0 | FMH_EHH_GAP1)));
    for (int a = 0; a < 2; ++a) {
      const uint64_t n_a = L.core[a], p0 = n_a * (n_a - (n_a ? 1 : 0)) / 2;
      if (!usable || p0 == 0) {
        o.ihh[a] = o.sl[a] = nan;
        continue;
      }
      // each: two u64 -> f64 conversions (exact or correctly rounded) and one division
      o.ihh[a] = (double)(L.area2[a] + R.area2[a]) / (double)(2 * p0);
      o.sl[a] = (double)(p0 + L.pair_steps[a] + R.pair_steps[a]) / (double)p0;
    }
    auto log_ratio = [nan](double one, double zero) { return (one > 0.0 && zero > 0.0) ? std::log(one / zero) : nan; };  // NaN compares false
    o.ihs = log_ratio(o.ihh[1], o.ihh[0]);
    o.nsl = log_ratio(o.sl[1], o.sl[0]);
  }
  return FMH_OK;
}
