// clump.hip — LD clumping: fmh_clump (participants, candidates and partner ranges on the host; a tile kernel that leaves one threshold bit per
// (candidate, participant of its window); the greedy rule over those bits on the host; the r^2 of every member with its index through
// fmh_geno_ld_pairs), fmh_geno_ld_pairs (the exact counts of arbitrary row pairs) and the host-only fmh_geno_ld_r2, fmh_geno_ld_pairs_host and
// fmh_clump_host.  Kernels in clump_kernels.hpp, host arithmetic in clump_host.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md
// section 3.23.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "clump_host.hpp"
#include "clump_kernels.hpp"
#include "geno_ld_call.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

// the pair kernel over P pairs of matrix rows (host lists), enqueued on the call's stream
int enqueue_pairs(StatCall& call, const fmh_matrix* m, const uint32_t* d_mask, uint32_t vec0, uint32_t vec1, const uint32_t* h_rows_a,
                  const uint32_t* h_rows_b, size_t P, fmh_geno_ld_counts* d_counts) {
  ClumpPairArgs a{};
  set_plane_rows(a, m);
  uint32_t *d_a = nullptr, *d_b = nullptr;
  FMH_TRY(call.upload(h_rows_a, P, &d_a));
  FMH_TRY(call.upload(h_rows_b, P, &d_b));
  a.mask = d_mask; a.vec0 = vec0; a.vec1 = vec1;
  a.rows_a = d_a; a.rows_b = d_b; a.P = (uint32_t)P; a.counts = d_counts;
  const size_t grid = wave_grid(P, call.ws->cus);
  hipLaunchKernelGGL(geno_ld_pairs_kernel, dim3((unsigned)grid), dim3(kClumpThreads), 0, call.st, a);
  HIP_TRY(hipGetLastError());
  return FMH_OK;
}

template <bool MISSING> int launch_tiles(const ClumpArgs& a, size_t n_items, int cus, hipStream_t st) {
  size_t grid = 0;
  FMH_TRY(persistent_grid(reinterpret_cast<const void*>(clump_ld_kernel<MISSING>), kClumpThreads, 0, n_items, cus, &grid, clump_lds_bytes(MISSING)));
  hipLaunchKernelGGL((clump_ld_kernel<MISSING>), dim3((unsigned)grid), dim3(kClumpThreads), 0, st, a);
  HIP_TRY(hipGetLastError());
  return FMH_OK;
}

}  // namespace

extern "C" int fmh_geno_ld_pairs(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, const uint32_t* h_rows_a,
                                 const uint32_t* h_rows_b, size_t P, fmh_geno_ld_counts* d_counts, void* stream) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  if (P != 0 && (!h_rows_a || !h_rows_b || !d_counts)) return fail(FMH_ERR_INVALID, "a NULL row list or output with %zu pairs", P);
  for (size_t i = 0; i < P; ++i)
    if (h_rows_a[i] >= m->variants || h_rows_b[i] >= m->variants)
      return fail(FMH_ERR_INVALID, "pair %zu names rows (%u, %u) of a matrix of %zu variants", i, h_rows_a[i], h_rows_b[i], m->variants);
  FMH_TRY(check_genotype_matrix(m, "genotype LD takes"));
  if (P > ((size_t)1 << 31)) return fail(FMH_ERR_UNSUPPORTED, "more than 2^31 work items: split the %zu pairs", P);
  if (P == 0) return FMH_OK;

  const ColumnMask mask = column_mask(m, h_samples_or_null, n_samples);
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  uint32_t* d_mask = nullptr;
  FMH_TRY(call.upload(mask.words.data(), mask.words.size(), &d_mask));
  FMH_TRY(call.start());
  FMH_TRY(enqueue_pairs(call, m, d_mask, mask.vec0, mask.vec1, h_rows_a, h_rows_b, P, d_counts));
  return call.finish();
}

extern "C" int fmh_clump(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                         const uint8_t* h_keep_or_null, const uint32_t* h_positions_or_null, const double* h_p, const fmh_clump_params* params,
                         uint32_t* h_index_of, double* h_r2_or_null, uint64_t* h_n_clumps_or_null, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (!h_p) return fail(FMH_ERR_INVALID, "NULL h_p");
  if (!h_index_of) return fail(FMH_ERR_INVALID, "NULL h_index_of");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  const fmh_clump_params& P = *params;
  if (const char* refused = clump_check_params(P)) return fail(FMH_ERR_INVALID, "%s (p1 %g, p2 %g, r2 %g)", refused, P.p1, P.p2, P.r2);
  if (const size_t bad = clump_bad_p(h_p, h_keep_or_null, row_count); bad != row_count)
    return fail(FMH_ERR_INVALID, "p %g of row entry %zu of the range is neither NaN nor within [0, 1]", h_p[bad], bad);
  const uint32_t* x = h_positions_or_null ? h_positions_or_null + row_begin : nullptr;
  for (size_t k = 1; x && k < row_count; ++k)
    if (x[k] < x[k - 1]) return fail(FMH_ERR_INVALID, "the positions descend at row entry %zu of the range", k);
  FMH_TRY(check_genotype_matrix(m, "LD clumping takes"));
  if (row_count >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "a range of %zu rows: fewer than 2^32 - 1 are taken (split the rows)", row_count);

  // ---- participants, candidates, partner ranges ----
  const ClumpPlan plan = clump_plan(h_keep_or_null, x, h_p, row_count, P);
  const size_t K = plan.rows.size(), n_cand = plan.cand.size();
  const bool missing = m->pc || m->p1 || m->p2;
  const size_t TC = clump_tile_candidates(missing);

  // ---- the threshold words: a candidate's bit row on the host covers the partner tiles its range meets; an item is a candidate tile x partner tile ----
  std::vector<size_t> word_at(n_cand + 1, 0);
  for (size_t c = 0; c < n_cand; ++c) word_at[c + 1] = word_at[c] + ((plan.hi[c] - 1) / kClumpTileP - plan.lo[c] / kClumpTileP + 1);
  const long long host_budget = options().clump_host_bytes.load(std::memory_order_relaxed);
  const long long budget = options().clump_budget_bytes.load(std::memory_order_relaxed);
  if (n_cand && (host_budget < 0 || word_at[n_cand] > (size_t)host_budget / sizeof(uint64_t)))
    return fail(FMH_ERR_UNSUPPORTED, "the threshold bits of %zu candidates need %zu bytes on the host, above FMH_CLUMP_HOST_BYTES = %lld", n_cand,
                word_at[n_cand] * sizeof(uint64_t), host_budget);
  const size_t n_tiles = (n_cand + TC - 1) / TC;
  std::vector<uint2> items;
  std::vector<size_t> item_at(n_tiles + 1, 0);  // the items of candidate tile T are [item_at[T], item_at[T + 1])
  for (size_t T = 0; T < n_tiles; ++T) {
    long long last = -1;  // lo and hi ascend with the candidate: so do the partner tiles
    for (size_t c = T * TC; c < std::min(n_cand, (T + 1) * TC); ++c)
      for (long long t = std::max<long long>(last + 1, plan.lo[c] / kClumpTileP); t <= (long long)((plan.hi[c] - 1) / kClumpTileP); ++t) {
        items.push_back(make_uint2((uint32_t)(T * TC), (uint32_t)t));
        last = t;
      }
    item_at[T + 1] = items.size();
    const size_t need = (item_at[T + 1] - item_at[T]) * TC * sizeof(uint64_t);
    if (budget < 0 || need > (size_t)budget)
      return fail(FMH_ERR_UNSUPPORTED, "the threshold words of %zu candidates and their windows need %zu bytes of scratch, above FMH_CLUMP_BUDGET_BYTES = %lld", TC,
                  need, budget);
  }
  if (items.size() > ((size_t)1 << 31)) return fail(FMH_ERR_UNSUPPORTED, "more than 2^31 work items (%zu tiles): split the rows", items.size());

  clump_fill_none(row_count, h_index_of, h_r2_or_null, h_n_clumps_or_null);
  if (K == 0 || n_cand == 0) return FMH_OK;  // no participant or no candidate: no launch

  // chunks of whole candidate tiles under the budget
  const size_t chunk_cap = (size_t)budget / (TC * sizeof(uint64_t));  // items of a launch; >= every tile's
  size_t max_items = 0;
  for (size_t T = 0, begin = 0; T < n_tiles; ++T) {
    if (item_at[T + 1] - item_at[begin] > chunk_cap) begin = T;
    max_items = std::max(max_items, item_at[T + 1] - item_at[begin]);
  }

  const ColumnMask mask = column_mask(m, h_samples_or_null, n_samples);
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  ClumpArgs a{};
  set_plane_rows(a, m);
  uint32_t *d_rows = nullptr, *d_mask = nullptr, *d_cand = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_sum = nullptr, *d_hom = nullptr;
  uint2* d_items = nullptr;
  unsigned long long* d_bits = nullptr;
  FMH_TRY(call.upload(plan.rows.data(), K, &d_rows));
  FMH_TRY(call.upload(mask.words.data(), mask.words.size(), &d_mask));
  FMH_TRY(call.upload(plan.cand.data(), n_cand, &d_cand));
  FMH_TRY(call.upload(plan.lo.data(), n_cand, &d_lo));
  FMH_TRY(call.upload(plan.hi.data(), n_cand, &d_hi));
  FMH_TRY(call.scratch.get(&d_items, max_items));
  FMH_TRY(call.scratch.get(&d_bits, max_items * TC));
  if (!missing) {
    FMH_TRY(call.scratch.get(&d_sum, K));
    FMH_TRY(call.scratch.get(&d_hom, K));
  }
  a.row_begin = row_begin;
  a.rows = d_rows; a.mask = d_mask; a.vec0 = mask.vec0; a.vec1 = mask.vec1;
  a.cand = d_cand; a.lo = d_lo; a.hi = d_hi;
  a.n_cand = (uint32_t)n_cand; a.K = (uint32_t)K; a.n = (uint32_t)n_samples;
  a.items = d_items; a.row_sum = d_sum; a.row_hom = d_hom; a.r2 = P.r2; a.bits = d_bits;

  std::vector<uint64_t> bits(word_at[n_cand], 0), chunk_bits(max_items * TC);
  bool first = true;
  for (size_t T = 0; T < n_tiles;) {
    size_t end = T + 1;
    while (end < n_tiles && item_at[end + 1] - item_at[T] <= chunk_cap) ++end;
    const size_t i0 = item_at[T], n_items = item_at[end] - i0;
    FMH_TRY(call.start());
    if (first && !missing) {
      hipLaunchKernelGGL(clump_row_sums_kernel, dim3((unsigned)wave_grid(K, call.ws->cus)), dim3(kClumpThreads), 0, st, a, d_sum, d_hom);
      HIP_TRY(hipGetLastError());
    }
    first = false;
    HIP_TRY(hipMemcpyAsync(d_items, items.data() + i0, n_items * sizeof(uint2), hipMemcpyHostToDevice, st));
    a.n_items = (uint32_t)n_items;
    FMH_TRY(missing ? launch_tiles<true>(a, n_items, call.ws->cus, st) : launch_tiles<false>(a, n_items, call.ws->cus, st));
    FMH_TRY(call.stop());
    HIP_TRY(hipMemcpyAsync(chunk_bits.data(), d_bits, n_items * TC * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FMH_TRY(call.finish());
    // the chunk's words into the candidates' bit rows
    for (size_t i = 0; i < n_items; ++i) {
      const uint2 item = items[i0 + i];
      for (size_t c = item.x; c < std::min<size_t>(n_cand, item.x + TC); ++c) {
        const size_t t_lo = plan.lo[c] / kClumpTileP, t_hi = (plan.hi[c] - 1) / kClumpTileP;
        if (item.y >= t_lo && item.y <= t_hi) bits[word_at[c] + (item.y - t_lo)] = chunk_bits[i * TC + (c - item.x)];
      }
    }
    T = end;
  }

  // ---- rule 3 over the bits ----
  std::vector<uint32_t> owner, indexes;
  clump_greedy(plan, [&](uint32_t c, uint32_t j) {
    const size_t t_lo = plan.lo[c] / kClumpTileP;
    return (bits[word_at[c] + (j / kClumpTileP - t_lo)] >> (j % kClumpTileP)) & 1ull;
  }, owner, indexes);
  clump_write_owners(plan, owner, h_index_of);
  if (h_n_clumps_or_null) *h_n_clumps_or_null = indexes.size();
  if (!h_r2_or_null) return FMH_OK;

  // ---- r^2 of every owned participant with its index ----
  std::vector<uint32_t> rows_a, rows_b, who;
  for (size_t j = 0; j < K; ++j)
    if (owner[j] != kClumpNone) {
      rows_a.push_back((uint32_t)(row_begin + plan.rows[owner[j]]));
      rows_b.push_back((uint32_t)(row_begin + plan.rows[j]));
      who.push_back(plan.rows[j]);
    }
  const size_t n_pairs = who.size();
  fmh_geno_ld_counts* d_counts = nullptr;
  FMH_TRY(call.scratch.get(&d_counts, n_pairs));
  std::vector<fmh_geno_ld_counts> counts(n_pairs);
  FMH_TRY(call.start());
  FMH_TRY(enqueue_pairs(call, m, d_mask, mask.vec0, mask.vec1, rows_a.data(), rows_b.data(), n_pairs, d_counts));
  FMH_TRY(call.stop());
  HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, n_pairs * sizeof(fmh_geno_ld_counts), hipMemcpyDeviceToHost, st));
  FMH_TRY(call.finish());
  for (size_t i = 0; i < n_pairs; ++i) h_r2_or_null[who[i]] = geno_ld_r2(counts[i]);
  return FMH_OK;
}

// ---- host only (no device) -------------------------------------------------------------------------------------------------------------------
extern "C" int fmh_geno_ld_r2(const fmh_geno_ld_counts* h_counts, size_t P, double* h_r2) {
  if (P != 0 && (!h_counts || !h_r2)) return fail(FMH_ERR_INVALID, "NULL counts or output with %zu records", P);
  for (size_t i = 0; i < P; ++i) h_r2[i] = geno_ld_r2(h_counts[i]);
  return FMH_OK;
}

namespace {
int check_dosage(const uint8_t* h_dosage, size_t K, size_t n) {
  if (n == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (K != 0 && !h_dosage) return fail(FMH_ERR_INVALID, "NULL dosage");
  for (size_t i = 0; i < K * n; ++i)
    if (h_dosage[i] > 3) return fail(FMH_ERR_INVALID, "dosage %u (row %zu, sample %zu) is not 0, 1, 2 or 3", h_dosage[i], i / n, i % n);
  return FMH_OK;
}
}  // namespace

extern "C" int fmh_geno_ld_pairs_host(const uint8_t* h_dosage, size_t K, size_t n, const uint32_t* h_rows_a, const uint32_t* h_rows_b, size_t P,
                                      fmh_geno_ld_counts* h_counts) {
  FMH_TRY(check_dosage(h_dosage, K, n));
  if (P != 0 && (!h_rows_a || !h_rows_b || !h_counts)) return fail(FMH_ERR_INVALID, "a NULL row list or output with %zu pairs", P);
  for (size_t i = 0; i < P; ++i)
    if (h_rows_a[i] >= K || h_rows_b[i] >= K) return fail(FMH_ERR_INVALID, "pair %zu names rows (%u, %u) of %zu rows", i, h_rows_a[i], h_rows_b[i], K);
  geno_ld_pairs_host(h_dosage, n, h_rows_a, h_rows_b, P, h_counts);
  return FMH_OK;
}

extern "C" int fmh_clump_host(const uint8_t* h_dosage, const uint32_t* h_x_or_null, const double* h_p, size_t K, size_t n, const fmh_clump_params* params,
                              uint32_t* h_index_of, double* h_r2_or_null, uint64_t* h_n_clumps_or_null) {
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (K != 0 && !h_p) return fail(FMH_ERR_INVALID, "NULL h_p");
  if (K != 0 && !h_index_of) return fail(FMH_ERR_INVALID, "NULL h_index_of");
  FMH_TRY(check_dosage(h_dosage, K, n));
  if (const char* refused = clump_check_params(*params)) return fail(FMH_ERR_INVALID, "%s (p1 %g, p2 %g, r2 %g)", refused, params->p1, params->p2, params->r2);
  if (const size_t bad = clump_bad_p(h_p, nullptr, K); bad != K) return fail(FMH_ERR_INVALID, "p %g of row %zu is neither NaN nor within [0, 1]", h_p[bad], bad);
  for (size_t k = 1; h_x_or_null && k < K; ++k)
    if (h_x_or_null[k] < h_x_or_null[k - 1]) return fail(FMH_ERR_INVALID, "the positions descend at row %zu", k);
  if (K >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "%zu rows: fewer than 2^32 - 1 are taken", K);
  clump_host(h_dosage, h_x_or_null, h_p, K, n, *params, h_index_of, h_r2_or_null, h_n_clumps_or_null);
  return FMH_OK;
}
