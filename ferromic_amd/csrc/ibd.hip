// ibd.hip — IBD segments: fmh_ibd_scan (per pair of diploid samples the qualifying runs of kept rows without a discordant genotype, exact
// integers from the bit planes: a states kernel that builds a sample-major bit image, a pair kernel over (row block, 32 x 32 pair tile)
// items that leaves one record per (block, pair), and a stitch kernel that joins the blocks and writes the [n][n] tables), its host twin
// fmh_ibd_scan_host, and the host-only fmh_ibd_sort_segments.  Kernels in ibd_kernels.hpp, host arithmetic in ibd_host.hpp, what it shares
// with the runs of homozygosity in segment_*.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.22.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "ibd_host.hpp"
#include "ibd_kernels.hpp"
#include "segment_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

const fmh_ibd_out kIbdNoTables{nullptr, nullptr, nullptr, nullptr};

bool any_table(const fmh_ibd_out& o) { return o.d_n_segments || o.d_sum_sites || o.d_sum_length || o.d_longest_length; }

int check_ibd_params(const fmh_ibd_params& p) {
  if (const char* refused = ibd_check_params(p)) return fail(FMH_ERR_INVALID, "%s (mode %u)", refused, p.mode);
  return FMH_OK;
}

template <uint32_t MODE, bool CALLED>
int launch_pairs(const IbdArgs& a, size_t grid, hipStream_t st) {
  hipLaunchKernelGGL((ibd_pair_kernel<MODE, CALLED>), dim3((unsigned)grid), dim3(kIbdThreads), 0, st, a);
  HIP_TRY(hipGetLastError());
  return FMH_OK;
}

int launch_pair_kernel(uint32_t mode, bool called, const IbdArgs& a, size_t grid, hipStream_t st) {
  if (mode == FMH_IBD1) return called ? launch_pairs<FMH_IBD1, true>(a, grid, st) : launch_pairs<FMH_IBD1, false>(a, grid, st);
  return called ? launch_pairs<FMH_IBD2, true>(a, grid, st) : launch_pairs<FMH_IBD2, false>(a, grid, st);
}

const void* pair_kernel(uint32_t mode, bool called) {
  if (mode == FMH_IBD1) return called ? reinterpret_cast<const void*>(ibd_pair_kernel<FMH_IBD1, true>) : reinterpret_cast<const void*>(ibd_pair_kernel<FMH_IBD1, false>);
  return called ? reinterpret_cast<const void*>(ibd_pair_kernel<FMH_IBD2, true>) : reinterpret_cast<const void*>(ibd_pair_kernel<FMH_IBD2, false>);
}

}  // namespace

extern "C" int fmh_ibd_scan(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                            const uint8_t* h_keep_or_null, const uint32_t* h_positions_or_null, const fmh_ibd_params* params,
                            const fmh_ibd_out* out_or_null, fmh_ibd_segment* d_segments_or_null, size_t segment_capacity, uint64_t* h_segment_count,
                            void* stream) {
  // ---- every refusal, before any launch ----
  const fmh_ibd_out out = out_or_null ? *out_or_null : kIbdNoTables;
  FMH_TRY(check_segment_scan(m, params, h_samples_or_null, n_samples, row_begin, row_count, h_positions_or_null, any_table(out), d_segments_or_null,
                             h_segment_count, "IBD segments", [&] { return check_ibd_params(*params); }));
  const fmh_ibd_params& P = *params;

  // ---- the kept rows and their positions ----
  const size_t n = n_samples;
  SegmentFrame frame(h_keep_or_null, h_positions_or_null, row_begin, row_count, h_samples_or_null, n);
  const size_t K = frame.kept.rows.size(), words = (K + 63) / 64;
  const bool segments = d_segments_or_null || h_segment_count;
  const size_t capacity = d_segments_or_null ? segment_capacity : 0;

  // ---- the scratch and the work items: refused before anything is enqueued ----
  const bool called = SegmentFrame::has_flags(m);
  const size_t n_planes = called ? 3 : 2;
  const size_t tiles_1d = (n + kIbdTile - 1) / kIbdTile, spad = tiles_1d * kIbdTile;
  const size_t n_tiles = tiles_1d * (tiles_1d + 1) / 2, slots = n_tiles * kIbdTileSlots;
  const size_t t_bytes = n_planes * words * spad * sizeof(unsigned long long), block_bytes = slots * kIbdRecBytes;
  const long long budget = options().ibd_budget_bytes.load(std::memory_order_relaxed);
  const long long forced_rows = options().ibd_item_rows.load(std::memory_order_relaxed);
  const bool work = K != 0 && n > 1;
  size_t max_blocks = 1;
  if (work) {
    const size_t forced_item = forced_rows > 0 ? ibd_item_rows(forced_rows, K, 1, 1, 1) : K;  // no forced size: one block has to fit
    const size_t need = t_bytes + (K + forced_item - 1) / forced_item * block_bytes;
    if (budget < 0 || need > (size_t)budget)
      return fail(FMH_ERR_UNSUPPORTED, "IBD segments of %zu samples over %zu kept rows need %zu bytes of scratch, above FMH_IBD_BUDGET_BYTES = %lld", n, K,
                  need, budget);
    max_blocks = ((size_t)budget - t_bytes) / block_bytes;
  }

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  if (h_segment_count) *h_segment_count = 0;
  if (!work) {  // no kept row or no pair: zero tables
    FMH_TRY(call.start());
    for (unsigned long long* t : {out.d_n_segments, out.d_sum_sites, out.d_sum_length, out.d_longest_length})
      if (t) HIP_TRY(hipMemsetAsync(t, 0, n * n * sizeof(unsigned long long), st));
    return call.finish();
  }

  const void* kernel = pair_kernel(P.mode, called);
  size_t full_grid = 0;
  FMH_TRY(persistent_grid(kernel, kIbdThreads, 0, (size_t)1 << 31, call.ws->cus, &full_grid, n_planes * kIbdBatch * 64 * sizeof(unsigned long long)));
  const size_t item_rows = ibd_item_rows(forced_rows, K, n_tiles, full_grid, max_blocks);
  const size_t n_blocks = (K + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(n_blocks * n_tiles, "FMH_IBD_ITEM_ROWS"));
  const size_t grid = std::min(full_grid, n_blocks * n_tiles);

  uint32_t* rec32 = nullptr;
  unsigned long long *rec64 = nullptr, *d_t = nullptr;
  const std::vector<unsigned long long> brk = break_bitmap(frame.kept.x, P.max_gap, 0, words);  // break(k) at bit k; read until the call ends
  FMH_TRY(frame.upload(call, m, brk, segments));
  FMH_TRY(call.scratch.get(&d_t, n_planes * words * spad));
  FMH_TRY(call.scratch.get(&rec32, n_blocks * IbdRec::n32 * slots));
  FMH_TRY(call.scratch.get(&rec64, n_blocks * kSegRec64 * slots));

  IbdStateArgs s{};
  set_plane_rows(s, m);
  s.nvec = frame.nvec;
  s.groups = frame.groups;
  s.row_begin = row_begin;
  s.rows = frame.d_rows;
  s.flags = frame.d_flags;
  s.rank = frame.d_rank;
  s.K = (uint32_t)K;
  s.words = (uint32_t)words;
  s.n_planes = (uint32_t)n_planes;
  s.n_items = (uint64_t)words * frame.groups;
  s.spad = spad;
  s.T = d_t;

  IbdArgs a{};
  a.T = d_t;
  a.spad = spad;
  a.words = (uint32_t)words;
  a.rows = frame.d_rows;
  a.x = frame.d_x;
  a.brk = frame.d_brk;
  a.n = (uint32_t)n;
  a.K = (uint32_t)K;
  a.item_rows = (uint32_t)item_rows;
  a.n_blocks = (uint32_t)n_blocks;
  a.n_tiles = (uint32_t)n_tiles;
  a.n_items = (uint32_t)(n_blocks * n_tiles);
  a.P = P;
  a.rec32 = rec32;
  a.rec64 = rec64;
  a.segments = d_segments_or_null;
  a.capacity = capacity;
  a.counter = frame.d_counter;
  a.out = out;

  FMH_TRY(call.start());
  HIP_TRY(hipMemsetAsync(d_t, 0, t_bytes, st));  // the padding samples' words; the states kernel writes the selected samples'
  FMH_TRY(frame.launch_flags(call, m, row_begin));
  {
    size_t state_grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(ibd_states_kernel), kIbdThreads, 0, (size_t)std::min<uint64_t>(s.n_items, (uint64_t)1 << 31),
                            call.ws->cus, &state_grid, 3 * 64 * 4 * sizeof(uint4)));
    hipLaunchKernelGGL(ibd_states_kernel, dim3((unsigned)state_grid), dim3(kIbdThreads), 0, st, s);
    HIP_TRY(hipGetLastError());
  }
  FMH_TRY(launch_pair_kernel(P.mode, called, a, grid, st));
  hipLaunchKernelGGL(ibd_stitch_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  return frame.finish(call, h_segment_count);
}

// ---- host only (no device) -------------------------------------------------------------------------------------------------------------------
extern "C" int fmh_ibd_scan_host(const uint8_t* h_dosage, const uint32_t* h_x_or_null, size_t n_kept, size_t n_samples, const fmh_ibd_params* params,
                                 const fmh_ibd_out* out_or_null, fmh_ibd_segment* h_segments_or_null, size_t segment_capacity,
                                 uint64_t* h_segment_count) {
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (n_kept != 0 && !h_dosage) return fail(FMH_ERR_INVALID, "NULL dosage");
  const fmh_ibd_out out = out_or_null ? *out_or_null : kIbdNoTables;
  FMH_TRY(check_ibd_params(*params));
  FMH_TRY(check_segment_request(h_x_or_null, n_kept, any_table(out), h_segments_or_null, h_segment_count));
  if (n_kept >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "%zu kept rows: fewer than 2^32 - 1 are taken", n_kept);
  for (size_t i = 0; i < n_kept * n_samples; ++i)
    if (h_dosage[i] > 3) return fail(FMH_ERR_INVALID, "dosage %u (kept row %zu, sample %zu) is not 0, 1, 2 or 3", h_dosage[i], i / n_samples, i % n_samples);
  ibd_scan_host(h_dosage, h_x_or_null, n_kept, n_samples, *params, out, h_segments_or_null, h_segments_or_null ? segment_capacity : 0, h_segment_count);
  return FMH_OK;
}

extern "C" int fmh_ibd_sort_segments(fmh_ibd_segment* h_segments, size_t count) {
  if (count != 0 && !h_segments) return fail(FMH_ERR_INVALID, "NULL segments");
  std::sort(h_segments, h_segments + count, ibd_segment_less);
  return FMH_OK;
}
