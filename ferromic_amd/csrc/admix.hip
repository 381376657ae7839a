// admix.hip — ancestry proportions by EM: the fmh_admix handle (fmh_admix_create: the per-row counts through fmh_genotype_counts, the usable
// rows, their 2-bit code image through grm_codes_kernel, the samples' site counts; fmh_admix_info, fmh_admix_destroy), fmh_admix_step (one EM
// step on the f64 matrix cores from the resident image) and the host-only fmh_admix_step_host, fmh_admix_start and fmh_admix_accelerate.
// Kernels in admix_kernels.hpp, host arithmetic in admix_host.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.27.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "abi_internal.hpp"
#include "admix_host.hpp"
#include "admix_kernels.hpp"
#include "geno_codes.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

struct fmh_admix {
  int device = 0;
  size_t n = 0, kept = 0, m = 0;
  size_t n_pad = 0, m_pad = 0, kwords = 0;  // samples and rows of the image; its 64-row words (m_pad / 64)
  unsigned long long* d_code = nullptr;     // [2][kwords][n_pad]
  uint32_t* d_sites = nullptr;              // [n] m_i
  std::vector<uint8_t> usable;              // per kept row
  std::vector<uint32_t> called, allele_count;
  std::vector<uint64_t> sample_sites;       // [n]
  ~fmh_admix() {
    if (d_code) pool_free(device, d_code);
    if (d_sites) pool_free(device, d_sites);
  }
};

namespace {

// stage times of the calling thread's last timed fmh_admix_step: the padded state, the step kernel, the reduce (ms)
thread_local double g_admix_stage_ms[3] = {0.0, 0.0, 0.0};

size_t image_bytes(size_t rows, size_t n_pad) { return 2 * (round_up(rows, kAdmixPassRows) / 64) * n_pad * sizeof(unsigned long long); }

}  // namespace

extern "C" int fmh_timing_read_admix(double* h_stage_ms) {
  if (!h_stage_ms) return fail(FMH_ERR_INVALID, "h_stage_ms is NULL");
  for (int i = 0; i < 3; ++i) h_stage_ms[i] = g_admix_stage_ms[i];
  return FMH_OK;
}

extern "C" int fmh_admix_create(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                                const uint8_t* h_keep_or_null, fmh_admix** out, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!out) return fail(FMH_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "admixture takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_packed(m, "admixture reads"));
  if (row_count >= 0xFFFFFF00ull) return fail(FMH_ERR_UNSUPPORTED, "a range of %zu rows: fewer than 2^32 - 256 are taken (split the rows)", row_count);
  const size_t n = n_samples;
  if (n > ((size_t)1 << 24)) return fail(FMH_ERR_UNSUPPORTED, "admixture of %zu samples: more than 2^24 samples are not supported", n);

  std::vector<uint32_t> kept_rows;
  kept_rows.reserve(row_count);
  for (size_t i = 0; i < row_count; ++i)
    if (!h_keep_or_null || h_keep_or_null[i]) kept_rows.push_back((uint32_t)i);
  const size_t kept = kept_rows.size();
  const size_t n_pad = round_up(n, 16);
  const size_t budget = (size_t)options().admix_budget_bytes.load();
  // with every kept row taken as usable (how many are is known only after the counting kernel)
  if (image_bytes(kept, n_pad) + 3 * row_count * sizeof(uint32_t) > budget)
    return fail(FMH_ERR_UNSUPPORTED, "the genotype image of %zu samples x %zu rows needs %zu bytes of device memory, budget %zu (FMH_ADMIX_BUDGET_BYTES)", n, kept,
                image_bytes(kept, n_pad) + 3 * row_count * sizeof(uint32_t), budget);

  std::unique_ptr<fmh_admix> h(new fmh_admix);
  h->device = m->device;
  h->n = n;
  h->kept = kept;
  h->n_pad = n_pad;
  h->usable.assign(kept, 0);
  h->called.assign(kept, 0);
  h->allele_count.assign(kept, 0);
  h->sample_sites.assign(n, 0);
  if (kept == 0) { *out = h.release(); return FMH_OK; }

  // ---- c, a of the kept rows: genotype QC's site tracks over the range ----
  FMH_TRY(use_device(m->device));
  {
    DeviceScratch scratch(m->device, (hipStream_t)stream);
    uint32_t* d_tracks = nullptr;
    FMH_TRY(scratch.get(&d_tracks, 3 * row_count));
    const fmh_genotype_site_out site{d_tracks, d_tracks + row_count, d_tracks + 2 * row_count};
    FMH_TRY(fmh_genotype_counts(m, h_samples_or_null, n, row_begin, row_count, nullptr, nullptr, &site, nullptr, nullptr, stream));
    scratch.settled = true;  // fmh_genotype_counts has synchronised the stream
    std::vector<uint32_t> tracks(3 * row_count);
    HIP_TRY(hipMemcpy(tracks.data(), d_tracks, tracks.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < kept; ++k) {
      const size_t r = kept_rows[k];
      h->called[k] = tracks[r] + tracks[row_count + r] + tracks[2 * row_count + r];
      h->allele_count[k] = tracks[row_count + r] + 2 * tracks[2 * row_count + r];
    }
  }
  std::vector<uint32_t> rows;
  for (size_t k = 0; k < kept; ++k) {
    h->usable[k] = fmh_host::admix_usable(h->called[k], h->allele_count[k]) ? 1 : 0;
    if (h->usable[k]) rows.push_back(kept_rows[k]);
  }
  const size_t M = rows.size();
  h->m = M;
  if (M == 0) { *out = h.release(); return FMH_OK; }

  // ---- the code image of the usable rows and the samples' site counts ----
  h->m_pad = round_up(M, kAdmixPassRows);
  h->kwords = h->m_pad / 64;
  const size_t words = (M + 63) / 64;
  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t nvec = last / 64 + 1, groups = (nvec + 3) / 4;  // 16-byte vectors through the last selected sample: within the row
  std::vector<uint32_t> rank((size_t)groups * kSegGroupSamples, kSegNone);
  for (size_t i = 0; i < n; ++i) rank[h_samples_or_null ? h_samples_or_null[i] : i] = (uint32_t)i;

  const size_t code_words = 2 * h->kwords * n_pad;
  void* p = nullptr;
  HIP_TRY(pool_malloc(m->device, &p, code_words * sizeof(unsigned long long)));
  h->d_code = (unsigned long long*)p;
  HIP_TRY(pool_malloc(m->device, &p, n * sizeof(uint32_t)));
  h->d_sites = (uint32_t*)p;

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  uint32_t *d_rows = nullptr, *d_rank = nullptr;
  uint8_t* d_flags = nullptr;
  FMH_TRY(call.upload(rows.data(), M, &d_rows));
  FMH_TRY(call.upload(rank.data(), rank.size(), &d_rank));
  const bool has_flags = m->pc || m->p1 || m->p2;
  if (has_flags) FMH_TRY(call.scratch.get(&d_flags, M));

  GrmCodeArgs a{};
  set_plane_rows(a, m);
  a.nvec = nvec;
  a.groups = groups;
  a.row_begin = row_begin;
  a.rows = d_rows;
  a.flags = d_flags;
  a.rank = d_rank;
  a.K = (uint32_t)M;
  a.words = (uint32_t)words;
  a.n_items = (uint64_t)words * groups;
  a.spad = n_pad;
  a.plane_words = h->kwords * n_pad;
  a.code = h->d_code;

  FMH_TRY(call.start());
  // the padding samples' and padding words' codes: both bits set = not called
  HIP_TRY(hipMemsetAsync(h->d_code, 0xFF, code_words * sizeof(unsigned long long), st));
  if (has_flags) {
    PlaneRows planes{};
    set_plane_rows(planes, m);
    hipLaunchKernelGGL(plane_flags_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, planes, row_begin, d_rows, (uint32_t)M, d_flags);
    HIP_TRY(hipGetLastError());
  }
  {
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(grm_codes_kernel), kGrmCodeThreads, 0, (size_t)std::min<uint64_t>(a.n_items, (uint64_t)1 << 31),
                            call.ws->cus, &grid, 2 * 64 * 4 * sizeof(uint4)));
    hipLaunchKernelGGL(grm_codes_kernel, dim3((unsigned)grid), dim3(kGrmCodeThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(admix_sites_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->d_code, h->kwords, n_pad, (uint32_t)n, h->d_sites);
  HIP_TRY(hipGetLastError());
  FMH_TRY(call.finish());
  std::vector<uint32_t> sites(n);
  HIP_TRY(hipMemcpy(sites.data(), h->d_sites, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) h->sample_sites[i] = sites[i];
  *out = h.release();
  return FMH_OK;
}

extern "C" int fmh_admix_info(const fmh_admix* h, fmh_admix_info_out* info) {
  if (!h || !info) return fail(FMH_ERR_INVALID, "NULL argument");
  info->n_samples = h->n;
  info->kept_rows = h->kept;
  info->usable_rows = h->m;
  info->h_usable = h->usable.data();
  info->h_called = h->called.data();
  info->h_allele_count = h->allele_count.data();
  info->h_sample_sites = h->sample_sites.data();
  return FMH_OK;
}

extern "C" void fmh_admix_destroy(fmh_admix* h) { delete h; }

extern "C" int fmh_admix_step(const fmh_admix* h, size_t n_components, const double* d_q, const double* d_f, double* d_q_out, double* d_f_out,
                              double* h_loglik_or_null, uint32_t flags, void* stream) {
  // ---- every refusal, before any launch ----
  if (!h) return fail(FMH_ERR_INVALID, "NULL handle");
  const size_t K = n_components;
  if (K < 1 || K > fmh_host::kAdmixMaxK) return fail(FMH_ERR_INVALID, "%zu components: 1 to %zu are taken", K, fmh_host::kAdmixMaxK);
  if (!d_q || !d_f || !d_q_out || !d_f_out) return fail(FMH_ERR_INVALID, "NULL state or output");
  if (d_q == d_q_out || d_f == d_f_out) return fail(FMH_ERR_INVALID, "input and output must not alias");
  if (flags & ~(FMH_ADMIX_UPDATE_Q | FMH_ADMIX_UPDATE_F)) return fail(FMH_ERR_INVALID, "unknown flag bits %#x", flags);
  const size_t n = h->n, M = h->m, n_pad = h->n_pad;

  // rows per item: the option (in whole passes), else so that every compute unit has two items; fewer items where the slabs would pass the budget
  const size_t budget = (size_t)options().admix_budget_bytes.load();
  const size_t image = 2 * h->kwords * n_pad * sizeof(unsigned long long);
  const size_t pads = (n_pad + h->m_pad) * kAdmixComps * sizeof(double);
  const size_t slab_item = n_pad * kAdmixComps * sizeof(double) + sizeof(double);
  size_t item_rows = kAdmixPassRows, n_items = 0;
  if (M != 0) {
    Workspace* w = nullptr;
    FMH_TRY(use_device(h->device));
    FMH_TRY(workspace(h->device, &w));
    const long long opt = options().admix_item_rows.load(std::memory_order_relaxed);
    if (opt > 0) {
      item_rows = round_up(std::min<size_t>((size_t)opt, kMaxItemRows), kAdmixPassRows);
    } else {
      const size_t wanted = 2 * (size_t)std::max(w->cus, 1);
      item_rows = std::max<size_t>(round_up((M + wanted - 1) / wanted, kAdmixPassRows), kAdmixPassRows);
      while (item_rows < h->m_pad && image + pads + ((M + item_rows - 1) / item_rows) * slab_item > budget) item_rows *= 2;
    }
    n_items = (M + item_rows - 1) / item_rows;
    if (image + pads + n_items * slab_item > budget)
      return fail(FMH_ERR_UNSUPPORTED, "a step on %zu samples x %zu usable rows in %zu items needs %zu bytes of device memory, budget %zu (FMH_ADMIX_BUDGET_BYTES)", n,
                  M, n_items, image + pads + n_items * slab_item, budget);
    FMH_TRY(check_item_count(n_items, "FMH_ADMIX_ITEM_ROWS"));
  }

  StatCall call;
  FMH_TRY(call.begin(h->device, stream));
  hipStream_t st = call.st;
  if (M == 0) {
    // no usable row: Q is copied, F has no entry, l = 0
    FMH_TRY(call.start());
    HIP_TRY(hipMemcpyAsync(d_q_out, d_q, n * K * sizeof(double), hipMemcpyDeviceToDevice, st));
    FMH_TRY(call.finish());
    if (h_loglik_or_null) *h_loglik_or_null = 0.0;
    return FMH_OK;
  }

  double *d_qpad = nullptr, *d_fpad = nullptr, *d_slab = nullptr, *d_part = nullptr;
  FMH_TRY(call.scratch.get(&d_qpad, n_pad * kAdmixComps));
  FMH_TRY(call.scratch.get(&d_fpad, h->m_pad * kAdmixComps));
  FMH_TRY(call.scratch.get(&d_slab, n_items * n_pad * kAdmixComps));
  FMH_TRY(call.scratch.get(&d_part, n_items + 1));  // the items' log partials, then their sum

  AdmixArgs a{};
  a.code32 = reinterpret_cast<const uint32_t*>(h->d_code);
  a.plane_halves = h->kwords * n_pad * 2;
  a.n_pad = (uint32_t)n_pad;
  a.n_tiles = (uint32_t)(n_pad / 16);
  a.m = (uint32_t)M;
  a.K = (uint32_t)K;
  a.item_rows = (uint32_t)item_rows;
  a.n_items = (uint32_t)n_items;
  a.update_q = (flags & FMH_ADMIX_UPDATE_Q) ? 1u : 0u;
  a.update_f = (flags & FMH_ADMIX_UPDATE_F) ? 1u : 0u;
  a.q_pad = d_qpad;
  a.f_pad = d_fpad;
  a.f_out = d_f_out;
  a.slab = d_slab;
  a.ll_part = d_part;

  KernelTimer<4> stages;
  FMH_TRY(call.start());
  FMH_TRY(stages.start(st));
  hipLaunchKernelGGL(admix_pad_kernel, dim3((unsigned)((n_pad * kAdmixComps + 255) / 256)), dim3(256), 0, st, d_q, n, (uint32_t)K, n_pad, 0.0, d_qpad);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(admix_pad_kernel, dim3((unsigned)((h->m_pad * kAdmixComps + 255) / 256)), dim3(256), 0, st, d_f, M, (uint32_t)K, h->m_pad, 0.5, d_fpad);
  HIP_TRY(hipGetLastError());
  FMH_TRY(stages.mark(1, st));
  {
    const uint32_t ks = (uint32_t)((K + 3) / 4);
    const bool logs = h_loglik_or_null != nullptr;
    void (*kernel)(const AdmixArgs) = nullptr;
    switch (ks) {
      case 1: kernel = logs ? admix_step_kernel<1, true> : admix_step_kernel<1, false>; break;
      case 2: kernel = logs ? admix_step_kernel<2, true> : admix_step_kernel<2, false>; break;
      case 3: kernel = logs ? admix_step_kernel<3, true> : admix_step_kernel<3, false>; break;
      default: kernel = logs ? admix_step_kernel<4, true> : admix_step_kernel<4, false>; break;
    }
    size_t grid = 0;
    const size_t lds = (4 * 2 * 16 * 17 + 2 * 4 * 256 + kAdmixThreads) * sizeof(double);
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), kAdmixThreads, 0, n_items, call.ws->cus, &grid, lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kAdmixThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  FMH_TRY(stages.mark(2, st));
  hipLaunchKernelGGL(admix_reduce_kernel, dim3((unsigned)(n_pad / 16)), dim3(256), 0, st, d_slab, (uint32_t)n_items, (uint32_t)n_pad, (uint32_t)n, (uint32_t)K, d_q,
                     h->d_sites, a.update_q, d_q_out, d_part, h_loglik_or_null ? d_part + n_items : nullptr);
  HIP_TRY(hipGetLastError());
  FMH_TRY(stages.stop(st));
  FMH_TRY(call.stop());
  double ll = 0.0;
  if (h_loglik_or_null) HIP_TRY(hipMemcpyAsync(&ll, d_part + n_items, sizeof(double), hipMemcpyDeviceToHost, st));
  FMH_TRY(call.finish());
  for (int i = 0; i < 3; ++i) FMH_TRY(stages.elapsed(i, &g_admix_stage_ms[i]));
  if (h_loglik_or_null) *h_loglik_or_null = ll;
  return FMH_OK;
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ----------------------------------
extern "C" int fmh_admix_step_host(const uint8_t* h_dosage, size_t rows, size_t n, size_t n_components, const double* h_q, const double* h_f, double* h_q_out,
                                   double* h_f_out, double* h_loglik_or_null, uint32_t flags, const fmh_admix_tracks* tracks_or_null) {
  if (n == 0) return fail(FMH_ERR_INVALID, "n is 0");
  if (rows != 0 && !h_dosage) return fail(FMH_ERR_INVALID, "NULL dosage table");
  if (tracks_or_null) {
    const fmh_admix_tracks& t = *tracks_or_null;
    const size_t m = fmh_host::admix_tracks(h_dosage, rows, n, t.h_usable, t.h_called, t.h_allele_count, t.h_sample_sites);
    if (t.h_usable_rows) *t.h_usable_rows = m;
  }
  if (!h_q && !h_q_out && !h_f && !h_f_out) return FMH_OK;  // the tracks alone
  const size_t K = n_components;
  if (K < 1 || K > fmh_host::kAdmixMaxK) return fail(FMH_ERR_INVALID, "%zu components: 1 to %zu are taken", K, fmh_host::kAdmixMaxK);
  if (!h_q || !h_f || !h_q_out || !h_f_out) return fail(FMH_ERR_INVALID, "NULL state or output");
  if (h_q == h_q_out || h_f == h_f_out) return fail(FMH_ERR_INVALID, "input and output must not alias");
  if (flags & ~(FMH_ADMIX_UPDATE_Q | FMH_ADMIX_UPDATE_F)) return fail(FMH_ERR_INVALID, "unknown flag bits %#x", flags);
  fmh_host::admix_step_host(h_dosage, rows, n, K, h_q, h_f, h_q_out, h_f_out, h_loglik_or_null, flags);
  return FMH_OK;
}

extern "C" int fmh_admix_start(const uint32_t* h_called, const uint32_t* h_allele_count, size_t m, size_t n, size_t n_components, uint64_t seed, double* h_q,
                               double* h_f) {
  const size_t K = n_components;
  if (K < 1 || K > fmh_host::kAdmixMaxK) return fail(FMH_ERR_INVALID, "%zu components: 1 to %zu are taken", K, fmh_host::kAdmixMaxK);
  if ((n != 0 && !h_q) || (m != 0 && (!h_f || !h_called || !h_allele_count))) return fail(FMH_ERR_INVALID, "NULL argument");
  for (size_t j = 0; j < m; ++j)
    if (!fmh_host::admix_usable(h_called[j], h_allele_count[j]))
      return fail(FMH_ERR_INVALID, "row %zu (c = %u, a = %u) is not usable", j, h_called[j], h_allele_count[j]);
  fmh_host::admix_start(h_called, h_allele_count, m, n, K, seed, h_q, h_f);
  return FMH_OK;
}

extern "C" int fmh_admix_accelerate(const double* h_q0, const double* h_f0, const double* h_q1, const double* h_f1, const double* h_q2, const double* h_f2, size_t n,
                                    size_t m, size_t n_components, double* h_qa, double* h_fa, double* h_alpha) {
  const size_t K = n_components;
  if (K < 1 || K > fmh_host::kAdmixMaxK) return fail(FMH_ERR_INVALID, "%zu components: 1 to %zu are taken", K, fmh_host::kAdmixMaxK);
  if (!h_alpha) return fail(FMH_ERR_INVALID, "h_alpha is NULL");
  if ((n != 0 && (!h_q0 || !h_q1 || !h_q2 || !h_qa)) || (m != 0 && (!h_f0 || !h_f1 || !h_f2 || !h_fa))) return fail(FMH_ERR_INVALID, "NULL argument");
  *h_alpha = fmh_host::admix_accelerate(h_q0, h_f0, h_q1, h_f1, h_q2, h_f2, n, m, K, h_qa, h_fa);
  return FMH_OK;
}
