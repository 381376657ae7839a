// hap.hip — haplotype homozygosity windows: fmh_haplotype_windows (the identical-haplotype classes of one group per row window, as
// integers), fmh_haplotype_stats (Garud's H1, H12, H123, H2/H1 and haplotype diversity of a window record, host only) and
// fmh_haplotype_max_members.  Kernel in hap_kernels.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.13.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "abi_internal.hpp"
#include "hap_kernels.hpp"
#include "hap_launch.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

static_assert(sizeof(fmh_hap_window) == 24 && sizeof(HapWindow) == sizeof(fmh_hap_window), "fmh_hap_window is 24 bytes");

namespace {

// every refusal, in the header's order; none needs a device
int check_args(const fmh_matrix* m, const fmh_groups* g, const RowSpan* windows, size_t n_windows, const void* d_out, bool want_first) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!g) return fail(FMH_ERR_INVALID, "NULL groups");
  if (!windows) return fail(FMH_ERR_INVALID, "h_windows is NULL");
  if (!d_out) return fail(FMH_ERR_INVALID, "d_out is NULL");
  if (g->n_groups != 1) return fail(FMH_ERR_INVALID, "the haplotype windows take exactly 1 group, got %d", g->n_groups);
  if (g->device != m->device || g->columns != m->columns) return fail(FMH_ERR_INVALID, "the groups were not made for this matrix");
  if (g->sizes[0] == 0) return fail(FMH_ERR_INVALID, "group 0 has no member");
  FMH_TRY(check_row_spans(windows, n_windows, "window", m->variants));
  if (n_windows == 0) return fail(FMH_ERR_INVALID, "n_windows is 0");
  if (g->sizes[0] > kHapMaxMembers)
    return fail(FMH_ERR_UNSUPPORTED, "a group of %llu members exceeds the %u the haplotype kernel holds on chip (fmh_haplotype_max_members)",
                (unsigned long long)g->sizes[0], kHapMaxMembers);
  if (want_first && n_windows > ((size_t)1 << 32) / (size_t)g->sizes[0])
    return fail(FMH_ERR_UNSUPPORTED, "a partition table of %zu windows x %llu members exceeds 2^32 entries", n_windows, (unsigned long long)g->sizes[0]);
  return check_packed(m, "the haplotype windows read");
}

}  // namespace

extern "C" uint32_t fmh_haplotype_max_members(void) { return kHapMaxMembers; }

extern "C" int fmh_haplotype_windows(const fmh_matrix* m, const fmh_groups* g, const uint64_t* h_windows, size_t n_windows, fmh_hap_window* d_out,
                                     uint32_t* d_first_or_null, void* stream) {
  FMH_TRY(check_args(m, g, reinterpret_cast<const RowSpan*>(h_windows), n_windows, d_out, d_first_or_null != nullptr));
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

  // launch shape (hap_launch.hpp, stat_call.hpp; the kernel's 44-46 VGPRs never bound the workgroups a CU holds, so LDS and thread slots decide)
  const unsigned threads = hap_pick_threads(n, n_windows, call.ws->cus);
  size_t grid = 0;
  FMH_TRY(persistent_grid(nullptr, threads, lds_bytes, n_windows, call.ws->cus, &grid));

  uint32_t* d_cols = nullptr;
  unsigned long long* d_windows = nullptr;
  FMH_TRY(call.upload(cols.data(), cols.size(), &d_cols));
  FMH_TRY(call.upload(h_windows, n_windows * 2, &d_windows));

  HapArgs a{};
  set_plane_rows(a, m);
  a.cols = d_cols;
  a.n = n;
  a.touch_first = (cols.front() >> 5) * 4;
  a.touch_last = (cols.back() >> 5) * 4;
  a.windows = d_windows;
  a.n_windows = n_windows;
  a.out = reinterpret_cast<HapWindow*>(d_out);
  a.first = d_first_or_null;

  const int planes = m->p2 ? 3 : m->p1 ? 2 : 1;
  void (*kernel)(const HapArgs) = m->pc ? (planes == 3 ? hap_kernel<3, true> : planes == 2 ? hap_kernel<2, true> : hap_kernel<1, true>)
                                        : (planes == 3 ? hap_kernel<3, false> : planes == 2 ? hap_kernel<2, false> : hap_kernel<1, false>);
  if (lds_bytes > ((size_t)64 << 10))
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));

  FMH_TRY(call.start());
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds_bytes, call.st, a);
  HIP_TRY(hipGetLastError());
  return call.finish();
}

extern "C" int fmh_haplotype_stats(const fmh_hap_window* h_windows, size_t n_windows, uint64_t n, fmh_hap_stats_out* h_out) {
  if (!h_windows || !h_out) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n == 0 || n >= ((uint64_t)1 << 26)) return fail(FMH_ERR_INVALID, "n must be 1 .. 2^26 - 1, got %llu", (unsigned long long)n);
  // each value is ONE division of two integers of at most n^2 < 2^52 (the pooled sums are at most (c1 + c2 + ...)^2 = n^2): both convert exactly
  const uint64_t n2 = n * n;
  for (size_t w = 0; w < n_windows; ++w) {
    const fmh_hap_window& r = h_windows[w];
    const uint64_t c1 = r.top[0], c2 = r.top[1], c3 = r.top[2];
    if (r.sum_sq == 0 || r.sum_sq > n2 || c1 * c1 > r.sum_sq || c1 + c2 + c3 > n)
      return fail(FMH_ERR_INVALID, "window %zu is not a partition of %llu members", w, (unsigned long long)n);
    fmh_hap_stats_out& o = h_out[w];
    o.h1 = (double)r.sum_sq / (double)n2;
    o.h12 = (double)(r.sum_sq + 2 * c1 * c2) / (double)n2;
    o.h123 = (double)(r.sum_sq + 2 * (c1 * c2 + c1 * c3 + c2 * c3)) / (double)n2;
    o.h2_h1 = (double)(r.sum_sq - c1 * c1) / (double)r.sum_sq;
    o.haplotype_diversity = n == 1 ? std::numeric_limits<double>::quiet_NaN() : (double)(n2 - r.sum_sq) / (double)(n * (n - 1));
  }
  return FMH_OK;
}
