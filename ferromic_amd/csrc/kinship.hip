// kinship.hip — relatedness: fmh_kinship_counts (the four exact genotype-class tables of every sample pair, as self-Grams of class operand
// planes on the matrix cores), fmh_kinship_stats (KING-robust kinship and IBS distance from those integers, host only) and
// fmh_kinship_unrelated (the greedy unrelated subset, host only).  Kernels in kin_kernels.hpp, the Gram itself is pairwise_kernels.hpp's,
// sized and launched through gram_launch.hpp; definition in include/ferromic_hip.h, operand algebra in DESIGN.md section 3.16.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "abi_internal.hpp"
#include "pairwise_kernels.hpp"
#include "gram_launch.hpp"
#include "kin_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

extern "C" int fmh_kinship_counts(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                                  const uint8_t* h_keep_or_null, const fmh_kinship_out* out, uint64_t* h_kept_rows, void* stream) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!out) return fail(FMH_ERR_INVALID, "out is NULL");
  if (!out->d_both || !out->d_het_het || !out->d_ibs0 || !out->d_het_hom) return fail(FMH_ERR_INVALID, "a table of out is NULL");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "kinship takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  FMH_TRY(check_packed(m, "kinship reads"));
  const size_t n = n_samples;
  // a strictly ascending list that ends at n - 1 is 0 .. n-1: the identity takes the dword staging of the planes kernel, no list is uploaded
  const uint32_t* h_list = h_samples_or_null && h_samples_or_null[n - 1] != n - 1 ? h_samples_or_null : nullptr;
  // general: some genotype may be uncalled (a called plane, or an upper allele plane whose bit un-calls the genotype); else V = 1 - H
  const bool general = m->pc || m->p1 || m->p2;
  const size_t na = general ? 2 * n : n;  // rows of region A whose pairs are wanted; the all-ones row follows them
  // (n <= 2^28 first: (2n + 1)^2 * 8 + n^2 * 8 then stays below 2^62 and cannot wrap)
  if (n > ((size_t)1 << 28)) return fail(FMH_ERR_UNSUPPORTED, "kinship of %zu samples: more than 2^28 samples are not supported", n);
  const size_t scratch_bytes = general ? (2 * n + 1) * (2 * n + 1) * 8 + n * n * 8 : 2 * n * n * 8;
  const long long budget = options().kin_budget_bytes.load();
  if (scratch_bytes > (size_t)budget)
    return fail(FMH_ERR_UNSUPPORTED, "kinship of %zu samples needs %zu bytes of scratch, above FMH_KIN_BUDGET_BYTES = %lld", n, scratch_bytes, budget);
  FMH_TRY(use_device(m->device));
  // the kept rows: every row of the range, or those the mask keeps (as a list the planes kernel gathers through)
  std::vector<unsigned long long> kept_list;
  size_t kept = row_count;
  if (h_keep_or_null) {
    kept_list.reserve(row_count);
    for (size_t i = 0; i < row_count; ++i)
      if (h_keep_or_null[i]) kept_list.push_back(row_begin + i);
    kept = kept_list.size();
  }
  if (h_kept_rows) *h_kept_rows = kept;
  if (kept == 0) return FMH_OK;
  hipStream_t st = (hipStream_t)stream;
  const GramFormat gf = gram_format(true);  // -1, 0 and 1 are exact in e2m1
  const size_t n_pad_a = round_up(na + 1, kPdBig), n_pad_w = round_up(n, kPdBig);
  const size_t slab = gram_row_slab(gf, n_pad_a + n_pad_w, kept);
  Workspace* w = nullptr;
  FMH_TRY(workspace(m->device, &w));
  std::lock_guard<std::mutex> busy(w->in_use);
  uint8_t* planes = nullptr;
  FMH_TRY(gram_planes(w, (n_pad_a + n_pad_w) * slab / gf.spb, &planes));
  DeviceScratch scratch(m->device, st);
  unsigned long long *d_ga = nullptr, *d_ta = nullptr, *d_gw = nullptr, *d_rows = nullptr;
  uint32_t* d_samples = nullptr;
  FMH_TRY(scratch.get(&d_ga, na * na));
  FMH_TRY(scratch.get(&d_ta, na));
  FMH_TRY(scratch.get(&d_gw, n * n));
  HIP_TRY(hipMemsetAsync(d_ga, 0, na * na * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(d_ta, 0, na * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(d_gw, 0, n * n * sizeof(unsigned long long), st));
  if (h_keep_or_null) {
    FMH_TRY(scratch.get(&d_rows, kept));
    HIP_TRY(hipMemcpyAsync(d_rows, kept_list.data(), kept * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  }
  if (h_list) {
    FMH_TRY(scratch.get(&d_samples, n));
    HIP_TRY(hipMemcpyAsync(d_samples, h_list, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  KinPlanesArgs a{};
  a.p0 = m->p0; a.p1 = m->p1; a.p2 = m->p2; a.pc = m->pc;
  a.plane_pitch = m->plane_pitch;
  a.samples = d_samples;
  a.n = (uint32_t)n;
  a.general = general ? 1 : 0;
  a.n_pad_a = n_pad_a;
  a.n_pad_w = n_pad_w;
  a.layout = gf.layout;
  a.planes = planes;
  const size_t smem = 3 * gf.ksites * kKinRowBytes;
  hipError_t e = hipSuccess;
  GramStageTimer timer(st);
  for (size_t done = 0; done < kept && e == hipSuccess; done += slab) {
    if ((e = timer.mark(0)) != hipSuccess) break;
    const size_t rows = std::min(slab, kept - done);
    const size_t s_pad = round_up(rows, gf.ksites);
    const size_t k_bytes = s_pad / gf.spb;
    a.rows = d_rows ? d_rows + done : nullptr;
    a.row_first = row_begin + done;
    a.row_count = rows;
    a.s_pad = s_pad;
    a.w_offset = n_pad_a * k_bytes;
    const dim3 grid((unsigned)(s_pad / gf.ksites), (unsigned)(n_pad_w / kKinSb));
    if (gf.fp4) hipLaunchKernelGGL(kin_planes_kernel<true>, grid, dim3(256), smem, st, a);
    else hipLaunchKernelGGL(kin_planes_kernel<false>, grid, dim3(256), smem, st, a);
    if ((e = hipGetLastError()) != hipSuccess) break;
    // operand products are -1, 0 or 1: an item may take 2^24 sites on FP4, 2^31 - 1 on int8 (gram_plan)
    GramPlan plan_a, plan_w;
    if ((e = gram_plan(w, m->device, gf, n_pad_a, (uint32_t)na, k_bytes, 1, &plan_a)) != hipSuccess) break;
    if ((e = gram_plan(w, m->device, gf, n_pad_w, (uint32_t)n, k_bytes, 1, &plan_w)) != hipSuccess) break;
    if ((e = timer.mark(1)) != hipSuccess) break;
    if ((e = gram_launch(w, gf, plan_a, planes, 0, 1, 0, d_ga, d_ta, st)) != hipSuccess) break;
    if ((e = timer.mark(2)) != hipSuccess) break;
    if ((e = gram_launch(w, gf, plan_w, planes + a.w_offset, 0, 1, 0, d_gw, nullptr, st)) != hipSuccess) break;
  }
  if (e == hipSuccess) e = timer.mark(3);
  if (e == hipSuccess) {
    const size_t total = n * n;
    hipLaunchKernelGGL(kin_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_ga, d_ta, d_gw, (uint32_t)n, general ? 1 : 0,
                       (unsigned long long)kept, out->d_both, out->d_het_het, out->d_ibs0, out->d_het_hom);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = timer.mark(-1);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) timer.read();
  if (e != hipSuccess) return fail(FMH_ERR_HIP, "kinship counts failed: %s", hipGetErrorString(e));
  scratch.settled = true;
  return FMH_OK;
}

// ---- host estimators (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ------------------------
extern "C" int fmh_kinship_stats(const uint64_t* h_both, const uint64_t* h_het_het, const uint64_t* h_ibs0, const uint64_t* h_het_hom, size_t n,
                                 double* h_kinship, double* h_ibs_distance_or_null) {
  if (n == 0) return FMH_OK;
  if (!h_both || !h_het_het || !h_ibs0 || !h_het_hom || !h_kinship) return fail(FMH_ERR_INVALID, "NULL argument");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      const size_t ij = i * n + j, ji = j * n + i;
      const uint64_t het_i = h_het_het[ij] + h_het_hom[ij], het_j = h_het_het[ij] + h_het_hom[ji];
      const uint64_t mn = std::min(het_i, het_j);
      const uint64_t hom = h_het_hom[ij] + h_het_hom[ji];
      h_kinship[ij] = mn == 0 ? nan : 0.5 - (double)(hom + 4 * h_ibs0[ij]) / (double)(4 * mn);
      if (h_ibs_distance_or_null) h_ibs_distance_or_null[ij] = h_both[ij] == 0 ? nan : (double)(hom + 2 * h_ibs0[ij]) / (double)(2 * h_both[ij]);
    }
  return FMH_OK;
}

extern "C" int fmh_kinship_unrelated(const double* h_kinship, size_t n, double threshold, uint8_t* h_keep) {
  if (n == 0) return FMH_OK;
  if (!h_kinship || !h_keep) return fail(FMH_ERR_INVALID, "NULL argument");
  std::fill(h_keep, h_keep + n, (uint8_t)1);
  // partners[i]: remaining j != i with phi(i, j) > threshold (NaN never exceeds it)
  std::vector<size_t> partners(n, 0);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j)
      if (j != i && h_kinship[i * n + j] > threshold) ++partners[i];
  for (;;) {
    size_t worst = n, most = 0;
    for (size_t i = 0; i < n; ++i)
      if (h_keep[i] && partners[i] > 0 && partners[i] >= most) { most = partners[i]; worst = i; }  // the highest index on a tie
    if (worst == n) break;
    h_keep[worst] = 0;
    partners[worst] = 0;
    // a partner of the removed sample loses it; the matrix is read as given (row i, column worst)
    for (size_t i = 0; i < n; ++i)
      if (h_keep[i] && h_kinship[i * n + worst] > threshold) --partners[i];
  }
  return FMH_OK;
}
