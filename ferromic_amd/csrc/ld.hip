// ld.hip — linkage disequilibrium: fmh_ld_band (banded r^2 and its counts between a row and its next `band` rows, straight from the packed
// bit planes), fmh_ld_prune (forward greedy thinning by r^2, the band kernel in row chunks with only the threshold bits) and
// fmh_ld_prune_bits (the greedy rule alone, host only).  Kernels in ld_kernels.hpp; definition and tiling in DESIGN.md section 3.11.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "abi_internal.hpp"
#include "ld_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

// every refusal of fmh_ld_band / fmh_ld_prune that needs no device, in the header's order
int check_args(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, size_t partner_end, size_t band, double threshold) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (band == 0) return fail(FMH_ERR_INVALID, "band is 0");
  if (partner_end > m->variants) return fail(FMH_ERR_INVALID, "partner_end %zu exceeds the matrix's %zu variants", partner_end, m->variants);
  if (row_begin > partner_end || row_count > partner_end - row_begin)
    return fail(FMH_ERR_INVALID, "rows [%zu, %zu) exceed partner_end %zu", row_begin, row_begin + row_count, partner_end);
  if (std::isnan(threshold)) return fail(FMH_ERR_INVALID, "threshold is NaN");
  if (g) {
    if (g->n_groups != 1) return fail(FMH_ERR_INVALID, "linkage disequilibrium takes exactly one group, got %d", g->n_groups);
    if (g->device != m->device || g->columns != m->columns) return fail(FMH_ERR_INVALID, "the group was not made for this matrix");
  }
  return check_packed(m, "linkage disequilibrium reads");
}

// the band kernel over rows [row_begin, row_begin + row_count), enqueued on `st`, no synchronisation
int enqueue_band(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, size_t partner_end, size_t band, double threshold,
                 const fmh_ld_band_out& out, uint32_t* d_site_n, uint32_t* d_site_alt, hipStream_t st) {
  LdArgs a{};
  a.p0 = m->p0; a.p1 = m->p1; a.p2 = m->p2; a.pc = m->pc;
  a.plane_pitch = m->plane_pitch;
  if (g) {
    a.mask = reinterpret_cast<const uint8_t*>(g->mask_bits);  // group 0's row: one bit per column, zero beyond the row
    const bool any = g->vec_first[0] <= g->vec_last[0];
    a.vec_begin = any ? g->vec_first[0] : 0;
    a.vec_end = any ? g->vec_last[0] + 1 : 0;
    a.n_const = (uint32_t)g->sizes[0];
  } else {
    a.mask = nullptr;
    a.vec_begin = 0;
    a.vec_end = m->pvec;
    a.n_const = m->columns;
  }
  a.partner_end = partner_end;
  a.band = band;
  a.over_words = (band + 31) / 32;
  a.threshold = threshold;
  const size_t d_tiles = (band + kLdBand - 1) / kLdBand;
  if (d_tiles > ((size_t)1 << 24)) return fail(FMH_ERR_UNSUPPORTED, "band %zu is too wide", band);
  a.d_tiles = (uint32_t)d_tiles;
  // a launch holds at most 2^30 tiles: whole row tiles per launch
  const size_t tiles_max = std::max<size_t>(((size_t)1 << 30) / d_tiles, 1);
  for (size_t done = 0; done < row_count;) {
    const size_t rows = std::min(row_count - done, tiles_max * kLdRows);
    a.row_begin = row_begin + done;
    a.row_end = a.row_begin + rows;
    a.r2 = out.r2 ? out.r2 + done * band : nullptr;
    a.n_ab = out.n_ab ? out.n_ab + done * band : nullptr;
    a.n_joint = out.n_joint ? out.n_joint + done * band : nullptr;
    a.over = out.over ? out.over + done * a.over_words : nullptr;
    a.site_n = d_site_n ? d_site_n + done : nullptr;
    a.site_alt = d_site_alt ? d_site_alt + done : nullptr;
    const dim3 grid((unsigned)(((rows + kLdRows - 1) / kLdRows) * d_tiles));
    if (m->pc) hipLaunchKernelGGL(ld_band_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(ld_band_kernel<false>, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    done += rows;
  }
  return FMH_OK;
}

// the greedy rule over rows [first, first + count) of a range of `total` rows; `over` holds the threshold bits of those rows
void greedy_rows(const uint32_t* over, size_t words, size_t band, size_t first, size_t count, size_t total, uint8_t* keep) {
  for (size_t r = 0; r < count; ++r) {
    const size_t i = first + r;
    if (!keep[i]) continue;  // a removed site removes nothing
    const uint32_t* row = over + r * words;
    for (size_t w = 0; w < words; ++w) {
      uint32_t bits = row[w];
      while (bits) {
        const size_t d = w * 32 + (size_t)__builtin_ctz(bits) + 1;
        bits &= bits - 1;
        if (d <= band && d < total - i) keep[i + d] = 0;
      }
    }
  }
}

// rows per chunk of fmh_ld_prune: the threshold bits of a chunk stay within 64 MiB of device scratch (and as much host memory)
constexpr size_t kLdPruneScratchBytes = (size_t)64 << 20;

}  // namespace

extern "C" int fmh_ld_band(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, size_t partner_end, size_t band,
                           double threshold, const fmh_ld_band_out* d_out, uint32_t* d_site_n, uint32_t* d_site_alt, void* stream) {
  if (!d_out) return fail(FMH_ERR_INVALID, "d_out is NULL");
  FMH_TRY(check_args(m, g, row_begin, row_count, partner_end, band, threshold));
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  if (row_count == 0) return FMH_OK;
  FMH_TRY(call.start());
  FMH_TRY(enqueue_band(m, g, row_begin, row_count, partner_end, band, threshold, *d_out, d_site_n, d_site_alt, call.st));
  return call.finish();
}

extern "C" int fmh_ld_prune_chunked(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, size_t window, double threshold,
                                    uint8_t* h_keep, size_t chunk_rows, void* stream) {
  if (row_count != 0 && !h_keep) return fail(FMH_ERR_INVALID, "h_keep is NULL");
  if (m) FMH_TRY(check_rows(row_begin, row_count, m->variants));
  const size_t end = row_begin + row_count;
  FMH_TRY(check_args(m, g, row_begin, row_count, end, window, threshold));  // (a NULL matrix is its first refusal)
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  if (row_count == 0) return FMH_OK;
  const size_t words = (window + 31) / 32;
  if (chunk_rows == 0) chunk_rows = std::max<size_t>(kLdPruneScratchBytes / (words * sizeof(uint32_t)), kLdRows);
  chunk_rows = std::min(chunk_rows, row_count);
  hipStream_t st = call.st;
  uint32_t* d_over = nullptr;
  FMH_TRY(call.scratch.get(&d_over, chunk_rows * words));
  std::vector<uint32_t> h_over(chunk_rows * words);
  std::fill(h_keep, h_keep + row_count, (uint8_t)1);
  fmh_ld_band_out out{};
  out.over = d_over;
  for (size_t done = 0; done < row_count; done += chunk_rows) {
    const size_t rows = std::min(chunk_rows, row_count - done);
    // pairs reach into the next chunks through partner_end = the end of the whole range; each chunk is one timed span
    FMH_TRY(call.start());
    FMH_TRY(enqueue_band(m, g, row_begin + done, rows, end, window, threshold, out, nullptr, nullptr, st));
    FMH_TRY(call.stop());
    HIP_TRY(hipMemcpyAsync(h_over.data(), d_over, rows * words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    FMH_TRY(call.finish());
    greedy_rows(h_over.data(), words, window, done, rows, row_count, h_keep);
  }
  return FMH_OK;
}

extern "C" int fmh_ld_prune(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, size_t window, double threshold,
                            uint8_t* h_keep, void* stream) {
  return fmh_ld_prune_chunked(m, g, row_begin, row_count, window, threshold, h_keep, 0, stream);
}

extern "C" int fmh_ld_prune_bits(const uint32_t* h_over, size_t row_count, size_t band, uint8_t* h_keep) {
  if (band == 0) return fail(FMH_ERR_INVALID, "band is 0");
  if (row_count == 0) return FMH_OK;
  if (!h_over || !h_keep) return fail(FMH_ERR_INVALID, "NULL argument");
  std::fill(h_keep, h_keep + row_count, (uint8_t)1);
  greedy_rows(h_over, (band + 31) / 32, band, 0, row_count, row_count, h_keep);
  return FMH_OK;
}
