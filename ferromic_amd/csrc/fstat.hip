// fstat.hip — Patterson's f-statistics: fmh_fstat_moments (per block of rows the usable rows, the sums of up to 32 groups' allele counts and
// of their pairwise products, exact u64 from the device), fmh_fstat_moment_count, and the two host-only halves: fmh_fstat_f4 (any f2 / f3 /
// f4 sum of one block from its slice, one exact 128-bit numerator and one division) and fmh_block_jackknife (the weighted delete-one-block
// jackknife).  Kernel in fstat_kernels.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.15.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "abi_internal.hpp"
#include "fstat_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

constexpr size_t kFstatDefaultItemRows = 4096;
// with 8 192 bytes of entries a workgroup's LDS stays under 20 KiB at any G (16 + 256 + 64 x 33 x 4 bytes of row state): eight workgroups per CU
constexpr size_t kFstatDefaultMaskBytes = 8192;
constexpr size_t kFstatMaxMaskBytes = (size_t)48 << 10;  // state + entries stay under the 64 KiB a launch gets without asking
constexpr uint64_t kFstatMaxSize = (uint64_t)1 << 17;    // fmh_fstat_f4: a term's cofactor n n stays at most 2^34

bool group_count_ok(int n_groups) { return n_groups >= 2 && n_groups <= FMH_FSTAT_MAX_GROUPS; }

}  // namespace

extern "C" size_t fmh_fstat_moment_count(int n_groups) {
  static_assert(FMH_FSTAT_MAX_GROUPS == kFstatMaxGroups, "the header's cap is the kernel's");
  if (!group_count_ok(n_groups)) return 0;
  const size_t G = (size_t)n_groups;
  return 1 + G + G * (G + 1) / 2;
}

extern "C" int fmh_fstat_moments(const fmh_matrix* m, const uint8_t* h_column_mask, int n_groups, const uint64_t* h_blocks, size_t n_blocks,
                                 uint64_t* d_moments, fmh_sfs_skipped* h_skipped, void* stream) {
  // ---- every refusal that needs no device, in the header's order ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!h_column_mask) return fail(FMH_ERR_INVALID, "h_column_mask is NULL");
  if (!h_blocks) return fail(FMH_ERR_INVALID, "h_blocks is NULL");
  if (!d_moments) return fail(FMH_ERR_INVALID, "d_moments is NULL");
  if (!group_count_ok(n_groups)) return fail(FMH_ERR_INVALID, "the f-statistics take 2 to %d groups, got %d", FMH_FSTAT_MAX_GROUPS, n_groups);
  const uint32_t G = (uint32_t)n_groups, columns = m->columns;
  uint64_t sizes[kFstatMaxGroups] = {0}, max_size = 0;
  for (uint32_t g = 0; g < G; ++g) {
    const uint8_t* row = h_column_mask + (size_t)g * columns;
    for (uint32_t c = 0; c < columns; ++c) sizes[g] += row[c] != 0;
    if (sizes[g] == 0) return fail(FMH_ERR_INVALID, "group %u has no member", g);
    max_size = std::max(max_size, sizes[g]);
  }
  const RowSpan* blocks = reinterpret_cast<const RowSpan*>(h_blocks);
  FMH_TRY(check_row_spans(blocks, n_blocks, "block", m->variants));
  if (n_blocks == 0) return fail(FMH_ERR_INVALID, "n_blocks is 0");
  for (size_t b = 0; b < n_blocks; ++b) {
    const unsigned __int128 worst = (unsigned __int128)(blocks[b].end - blocks[b].begin) * max_size * max_size;
    if (worst >= ((unsigned __int128)1 << 63))
      return fail(FMH_ERR_UNSUPPORTED, "block %zu: %zu rows x %llu^2 members reach 2^63, a u64 moment could wrap: use smaller blocks", b,
                  blocks[b].end - blocks[b].begin, (unsigned long long)max_size);
  }
  FMH_TRY(check_packed(m, "the f-statistics read"));

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  const size_t M = fmh_fstat_moment_count(n_groups);
  HIP_TRY(hipMemsetAsync(d_moments, 0, n_blocks * M * sizeof(uint64_t), st));
  if (h_skipped) memset(h_skipped, 0, n_blocks * sizeof(fmh_sfs_skipped));

  // work items: at most item_rows rows each, never across a block; a block is cut into EQUAL items (a 5 000-row block into 2 x 2 500, not
  // 4 096 + 904: with the uneven cut 2 000 such blocks measured 3.2 ms against 2.1 ms with items of 1 024 or of 16 384 rows)
  const size_t item_rows = item_rows_of(options().fstat_item_rows, kFstatDefaultItemRows);
  std::vector<FstatItem> items;
  for (size_t b = 0; b < n_blocks; ++b) {
    const size_t rows = blocks[b].end - blocks[b].begin;
    if (rows == 0) continue;
    const size_t pieces = (rows + item_rows - 1) / item_rows;
    FMH_TRY(check_item_count(items.size() + pieces, "FMH_FSTAT_ITEM_ROWS"));
    const size_t each = (rows + pieces - 1) / pieces;  // <= item_rows
    for (size_t r = blocks[b].begin; r < blocks[b].end; r += each)
      items.push_back(FstatItem{(unsigned long long)r, (uint32_t)std::min(each, blocks[b].end - r), (uint32_t)b});
  }
  if (items.empty()) {
    HIP_TRY(hipStreamSynchronize(st));
    return FMH_OK;
  }

  // the mask entries: per 16-byte vector of the union window the groups that have a member there, sorted by vector (CSR)
  const uint32_t pvec = m->pvec;
  std::vector<uint32_t> bits((size_t)G * pvec * 4, 0);  // [G][pvec] vectors of four dwords
  for (uint32_t g = 0; g < G; ++g) {
    const uint8_t* row = h_column_mask + (size_t)g * columns;
    uint32_t* out = bits.data() + (size_t)g * pvec * 4;
    for (uint32_t c = 0; c < columns; ++c)
      if (row[c]) out[c >> 5] |= 1u << (c & 31);
  }
  auto vector_has = [&](uint32_t g, uint32_t v) {
    const uint32_t* w = bits.data() + ((size_t)g * pvec + v) * 4;
    return (w[0] | w[1] | w[2] | w[3]) != 0;
  };
  uint32_t vec_begin = pvec, vec_end = 0;
  for (uint32_t v = 0; v < pvec; ++v)
    for (uint32_t g = 0; g < G; ++g)
      if (vector_has(g, v)) { vec_begin = std::min(vec_begin, v); vec_end = v + 1; break; }
  std::vector<uint32_t> ent_off, ent_group, ent_mask;
  ent_off.reserve(vec_end - vec_begin + 1);
  for (uint32_t v = vec_begin; v < vec_end; ++v) {
    ent_off.push_back((uint32_t)ent_group.size());
    for (uint32_t g = 0; g < G; ++g)
      if (vector_has(g, v)) {
        ent_group.push_back(g);
        const uint32_t* w = bits.data() + ((size_t)g * pvec + v) * 4;
        ent_mask.insert(ent_mask.end(), w, w + 4);
      }
  }
  ent_off.push_back((uint32_t)ent_group.size());
  const uint32_t n_entries = (uint32_t)ent_group.size(), n_vectors = vec_end - vec_begin;

  FstatArgs a{};
  set_plane_rows(a, m);
  a.vec_begin = vec_begin;
  a.vec_end = vec_end;
  a.n_groups = G;
  a.n_entries = n_entries;
  a.n_items = (uint32_t)items.size();
  a.slots = (uint32_t)M;
  a.moments = reinterpret_cast<unsigned long long*>(d_moments);

  // four lanes per row while the union window is at most four vectors, sixteen beyond (as the spectra); the entries in LDS while they fit
  const bool lanes4 = n_vectors <= 4;
  const uint32_t rows_per_pass = kFstatThreads / (lanes4 ? 4 : 16);
  const long long opt_bytes = options().fstat_lds_mask_bytes.load(std::memory_order_relaxed);
  const size_t budget = opt_bytes <= 0 ? kFstatDefaultMaskBytes : std::min<size_t>((size_t)opt_bytes, kFstatMaxMaskBytes);
  const size_t entry_bytes = (size_t)fstat_lds_entry_dwords(n_entries, n_vectors) * sizeof(uint32_t);
  const bool lds_masks = entry_bytes <= budget;
  const size_t lds_bytes = (size_t)fstat_lds_state_dwords(rows_per_pass, G) * sizeof(uint32_t) + (lds_masks ? entry_bytes : 0);
  void (*kernel)(const FstatArgs) = lanes4 ? (lds_masks ? fstat_kernel<4, true> : fstat_kernel<4, false>)
                                           : (lds_masks ? fstat_kernel<16, true> : fstat_kernel<16, false>);
  size_t grid = 0;
  FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), kFstatThreads, lds_bytes, items.size(), call.ws->cus, &grid));

  FstatItem* d_items = nullptr;
  uint32_t *d_off = nullptr, *d_group = nullptr;
  uint4* d_mask = nullptr;
  FMH_TRY(call.upload(items.data(), items.size(), &d_items));
  FMH_TRY(call.upload(ent_off.data(), ent_off.size(), &d_off));
  FMH_TRY(call.upload(ent_group.data(), ent_group.size(), &d_group));
  FMH_TRY(call.upload(ent_mask.data(), (size_t)n_entries, &d_mask));  // four dwords per entry
  unsigned long long* d_skipped = nullptr;
  if (h_skipped) FMH_TRY(call.zeroed(n_blocks * 2, &d_skipped));
  a.items = d_items;
  a.ent_off = d_off;
  a.ent_group = d_group;
  a.ent_mask = d_mask;
  a.skipped = d_skipped;

  FMH_TRY(call.start());
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kFstatThreads), lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  FMH_TRY(call.stop());
  static_assert(sizeof(fmh_sfs_skipped) == 2 * sizeof(unsigned long long), "fmh_sfs_skipped is two u64");
  if (h_skipped) HIP_TRY(hipMemcpyAsync(h_skipped, d_skipped, n_blocks * sizeof(fmh_sfs_skipped), hipMemcpyDeviceToHost, st));
  return call.finish();
}

// ---- host only ---------------------------------------------------------------------------------------------------------------------------
namespace {

// slot of the product moment of groups i and j in a slice
size_t pair_slot(size_t G, size_t i, size_t j) {
  if (i > j) std::swap(i, j);
  return 1 + G + i * G - i * (i - 1) / 2 + (j - i);
}

}  // namespace

extern "C" int fmh_fstat_f4(const uint64_t* h_moments, const uint64_t* h_sizes, int n_groups, int A, int B, int C, int D, int unbiased,
                            double* h_sum) {
  if (!h_moments || !h_sizes || !h_sum) return fail(FMH_ERR_INVALID, "NULL argument");
  if (!group_count_ok(n_groups)) return fail(FMH_ERR_INVALID, "the f-statistics take 2 to %d groups, got %d", FMH_FSTAT_MAX_GROUPS, n_groups);
  const int idx[4] = {A, B, C, D};
  for (int k = 0; k < 4; ++k) {
    if (idx[k] < 0 || idx[k] >= n_groups) return fail(FMH_ERR_INVALID, "group index %d is outside 0..%d", idx[k], n_groups - 1);
    if (h_sizes[idx[k]] == 0) return fail(FMH_ERR_INVALID, "group %d has sample size 0", idx[k]);
    if (h_sizes[idx[k]] > kFstatMaxSize) return fail(FMH_ERR_UNSUPPORTED, "sample size %llu of group %d exceeds 2^17", (unsigned long long)h_sizes[idx[k]], idx[k]);
  }
  const size_t G = (size_t)n_groups;
  using i128 = __int128;
  const i128 nA = (i128)h_sizes[A], nB = (i128)h_sizes[B], nC = (i128)h_sizes[C], nD = (i128)h_sizes[D];
  auto S = [&](int x, int y) { return (i128)h_moments[pair_slot(G, (size_t)x, (size_t)y)]; };
  // S_AC/(nA nC) - S_AD/(nA nD) - S_BC/(nB nC) + S_BD/(nB nD) over nA nB nC nD: moments are below 2^63, cofactors at most 2^34
  const i128 num = S(A, C) * nB * nD - S(A, D) * nB * nC - S(B, C) * nA * nD + S(B, D) * nA * nC;
  const i128 den = nA * nB * nC * nD;
  double sum = (double)num / (double)den;
  if (unbiased) {
    // h_X = (n_X S_X - S_XX) / (n_X^2 (n_X - 1)): the sum over the block of the unbiased estimate of p_X (1 - p_X) / n_X
    auto h = [&](int x) {
      const uint64_t n = h_sizes[x];
      if (n < 2) return std::numeric_limits<double>::quiet_NaN();
      const i128 hn = (i128)n * (i128)h_moments[1 + (size_t)x] - S(x, x);
      return (double)hn / (double)(n * n * (n - 1));  // the denominator is below 2^51: exact
    };
    if (A == C) sum -= h(A);
    if (A == D) sum += h(A);
    if (B == C) sum += h(B);
    if (B == D) sum -= h(B);
  }
  *h_sum = sum;
  return FMH_OK;
}

extern "C" int fmh_block_jackknife(const double* h_num, const double* h_den, const double* h_weight, size_t n_blocks, fmh_jackknife_out* h_out) {
  if (!h_num || !h_den || !h_out) return fail(FMH_ERR_INVALID, "NULL argument");
  const double* w = h_weight ? h_weight : h_den;
  for (size_t j = 0; j < n_blocks; ++j)
    if (!(w[j] >= 0.0) || std::isinf(w[j])) return fail(FMH_ERR_INVALID, "the weight of block %zu is negative or not finite", j);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  fmh_jackknife_out o{nan, nan, nan, nan, 0};
  double num = 0.0, den = 0.0, n = 0.0;
  for (size_t j = 0; j < n_blocks; ++j) {
    if (w[j] == 0.0) continue;
    ++o.blocks;
    num += h_num[j];
    den += h_den[j];
    n += w[j];
  }
  if (o.blocks == 0 || den == 0.0) { *h_out = o; return FMH_OK; }
  const double g = (double)o.blocks, theta = num / den;
  o.estimate = theta;
  if (o.blocks == 1) {  // the one block's weight in theta_J is 1 - m / n = 0: nothing is left to delete
    o.jackknife_estimate = theta;
    *h_out = o;
    return FMH_OK;
  }
  double drop_sum = 0.0;  // sum_j (1 - m_j / n) theta_(-j)
  for (size_t j = 0; j < n_blocks; ++j) {
    if (w[j] == 0.0) continue;
    const double theta_j = (num - h_num[j]) / (den - h_den[j]);
    drop_sum += (1.0 - w[j] / n) * theta_j;
  }
  o.jackknife_estimate = g * theta - drop_sum;
  double var = 0.0;
  for (size_t j = 0; j < n_blocks; ++j) {
    if (w[j] == 0.0) continue;
    const double theta_j = (num - h_num[j]) / (den - h_den[j]);
    const double h = n / w[j];
    const double tau = h * theta - (h - 1.0) * theta_j;
    const double d = tau - o.jackknife_estimate;
    var += d * d / (h - 1.0);
  }
  o.se = std::sqrt(var / g);
  o.z = theta / o.se;
  *h_out = o;
  return FMH_OK;
}
