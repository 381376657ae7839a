// roh_kernels.hpp — gfx950 kernels of the runs of homozygosity (roh.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md section
// 3.21).  The first statistic here whose work is a stateful scan ALONG rows for every sample.
//
// Scan (roh_scan_kernel).  A workgroup of 256 threads owns an item = (block of item_rows kept rows [b0, b1), group of 256 samples) on the
// persistent grid; thread t owns sample 256 g + t.  The item walks the VIRTUAL kept rows [s, b1 + W - 1), s = max(0, b0 - (W - 1)): the W - 1
// rows before the block fill the window history, the W - 1 past it complete the windows that cover the block's last rows (rows at or past K
// are fed as zeros and complete no window).  A step of 64 kept rows is fetched through the kept-row list, 16 bytes per thread and plane
// (thread = row of the step x 16-byte part of the group's 64 bytes; segment_kernels.hpp: plane_fetch, upper planes, row_gap / row_hi
// honoured through the per-kept-row flags of plane_flags_kernel), turned into `called` and `het` 2-bit fields and parked in LDS; the next
// step's loads are issued before the walk.  A lane gathers ITS bit of the 64 rows into two 64-bit masks and walks them with everything in registers:
//   hist_het / hist_miss: bit j = the state of row k - j;   hist_hom: bit j = whether window t = k - (W - 1) - j is homozygous
//   at virtual row k the window t = k - (W - 1) is complete (iff k - s >= W - 1 and k < K) and row d = k - (W - 1) is decided:
//   n_hom(d) = popcount(hist_hom & low W bits), n_cov(d) = min(d, K - W) - max(0, d - W + 1) + 1, its own state = bit W - 1 of the histories.
// k, d, n_cov, need[n_cov] and break(d) are the same for every lane: scalar work.  Runs strictly inside the block are judged, tallied and
// (when asked for) appended by the lane itself; per (block, sample) the item leaves the record of segment_kernels.hpp (SegRec<2>: head,
// tail and the interior tallies) and, behind its two u64 fields, the block's bins.
// Stitch (roh_stitch_kernel).  One thread per selected sample joins the blocks by the shared rule (seg_stitch), judges the joined runs,
// adds the interior tallies and bins in block order and writes the sample's tables: one writer per entry.  Segments are appended with a
// vector atomicAdd on a device counter, stored below the capacity (seg_append).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ferromic_hip.h"
#include "plane_rows.hpp"
#include "roh_host.hpp"  // roh_qualifies
#include "segment_kernels.hpp"

namespace fmh {

constexpr uint32_t kRohThreads = 256;
constexpr uint32_t kRohStepRows = 64;
using RohRec = SegRec<2>;                  // a run carries (het, miss)
constexpr uint32_t kRohRec64 = kSegRec64;  // length, longest; then bin_runs[n_bins], bin_length[n_bins]

struct RohArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t nvec;    // 16-byte vectors of a row through the last selected sample (<= plane_pitch / 16)
  uint32_t groups;  // sample groups: ceil(nvec / 4)
  size_t row_begin;
  const uint32_t* rows;            // [K] kept rows, relative to row_begin
  const uint8_t* flags;            // [K] bit 0: the called plane of the row is read, bit 1: the upper planes are; null = neither exists
  const uint32_t* x;               // [K] positions of the kept rows
  const unsigned long long* brk;   // break(k) at bit k + 64 (64 zero bits in front, zero words behind: any step's window is two whole words)
  const uint32_t* rank;            // [groups * 256] list position of a matrix sample, kSegNone where it is not selected
  const uint32_t* samples;         // [n] or null (entry i is sample i)
  uint32_t n, K, item_rows, n_blocks, n_items;
  fmh_roh_params P;
  uint32_t* rec32;                 // [n_blocks][RohRec::n32][groups * 256]
  unsigned long long* rec64;       // [n_blocks][kRohRec64 + 2 n_bins][groups * 256]
  fmh_roh_segment* segments;       // device, `capacity` elements, or null
  unsigned long long capacity;
  unsigned long long* counter;     // null = segments are neither counted nor stored
  fmh_roh_out out;
};

using fmh_host::roh_qualifies;  // the host twin's rule
__device__ __forceinline__ uint32_t roh_bin(const fmh_roh_params& P, uint64_t length) {
  uint32_t b = 0;
#pragma unroll
  for (uint32_t e = 0; e < 7; ++e) b += (e + 1 < P.n_bins && P.bin_edges[e] <= length) ? 1u : 0u;
  return b;
}
__device__ __forceinline__ void roh_append(const RohArgs& A, uint32_t rank, uint32_t first, uint32_t last, uint32_t n_het, uint32_t n_missing) {
  seg_append(A, [&] { return fmh_roh_segment{rank, last - first + 1, n_het, n_missing, A.rows[first], A.rows[last]}; });
}

// Launched with kRohThreads threads; static LDS: 2 x 4 KiB of fields + the need table.
static __global__ __launch_bounds__(kRohThreads) void roh_scan_kernel(const RohArgs A) {
  __shared__ uint4 s_cal4[kRohStepRows * 4];  // [row of the step][16-byte part]: a row's 16 words
  __shared__ uint4 s_het4[kRohStepRows * 4];
  const uint32_t* s_cal = reinterpret_cast<const uint32_t*>(s_cal4);
  const uint32_t* s_het = reinterpret_cast<const uint32_t*>(s_het4);
  __shared__ uint32_t s_need[65];
  const uint32_t tid = threadIdx.x;
  const uint32_t srow = tid >> 2, spart = tid & 3u;  // the staging thread's row of the step and 16-byte part of the group's 64 bytes
  const uint32_t word = tid >> 4, shift = 2u * (tid & 15u);  // the walking lane's word of a row's 16 and its field in it
  const uint32_t W = A.P.window, K = A.K, nb = A.P.n_bins;
  const uint64_t mask_w = W == 64 ? ~0ull : ((1ull << W) - 1ull);
  const uint32_t need_full = A.P.need[W];
  const size_t spad = (size_t)A.groups * kSegGroupSamples;
  if (tid < 65) s_need[tid] = A.P.need[tid];  // read after the first step's barriers

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t rb = it / A.groups, sg = it % A.groups;
    const uint32_t b0 = rb * A.item_rows, b1 = K - b0 < A.item_rows ? K : b0 + A.item_rows;
    const uint32_t s = b0 >= W - 1 ? b0 - (W - 1) : 0;
    const uint64_t end = (uint64_t)b1 + (W - 1);  // virtual rows [s, end)
    const uint32_t steps = (uint32_t)((end - s + kRohStepRows - 1) / kRohStepRows);
    const uint32_t vec = 4u * sg + spart;
    const bool inside = vec < A.nvec;  // a vector past the covered samples is zero
    const size_t slot = (size_t)sg * kSegGroupSamples + tid;
    const uint32_t rank = A.rank[slot];
    const bool active = rank != kSegNone;
    uint32_t* r32 = A.rec32 + (size_t)rb * RohRec::n32 * spad + slot;
    unsigned long long* r64 = A.rec64 + (size_t)rb * (kRohRec64 + 2 * nb) * spad + slot;
    if (active)
      for (uint32_t b = 0; b < 2 * nb; ++b) r64[(kRohRec64 + b) * spad] = 0;  // the bins are added to in place: one writer, this lane

    // the kept row of this thread in step j and its plane flags, one step ahead of the planes they address
    auto meta = [&](uint32_t j, uint32_t& row, uint32_t& fl) {
      const uint64_t k = (uint64_t)s + (uint64_t)j * kRohStepRows + srow;
      const uint32_t kk = k < K ? (uint32_t)k : K - 1;
      row = A.rows[kk];
      fl = A.flags ? (uint32_t)A.flags[kk] : 0u;
    };
    auto fetch = [&](uint32_t j, uint32_t row, uint32_t fl) {
      const uint64_t k = (uint64_t)s + (uint64_t)j * kRohStepRows + srow;
      const bool ok = inside && k < K;
      const size_t off = (A.row_begin + row) * A.plane_pitch + (size_t)(inside ? vec : 0) * 16;
      return plane_fetch(A, off, ok, fl);
    };

    // the lane's scan state
    uint64_t hist_het = 0, hist_miss = 0, hist_hom = 0;
    bool open = false;
    uint32_t first = 0, n_het = 0, n_miss = 0;
    uint32_t head_last = kSegNone, head_het = 0, head_miss = 0;
    uint32_t runs = 0, sites = 0;
    uint64_t length_sum = 0, longest = 0;

    auto close = [&](uint32_t last) {
      open = false;
      if (first == b0) {  // touches the block's first row: the stitch judges it
        head_last = last; head_het = n_het; head_miss = n_miss;
        return;
      }
      const uint64_t n_sites = last - first + 1, length = (uint64_t)A.x[last] - A.x[first] + 1;
      if (!roh_qualifies(A.P, n_sites, length, n_het, n_miss)) return;
      ++runs; sites += (uint32_t)n_sites; length_sum += length; longest = length > longest ? length : longest;
      if (nb) {
        const uint32_t b = roh_bin(A.P, length);
        r64[(kRohRec64 + b) * spad] += 1;
        r64[(kRohRec64 + nb + b) * spad] += length;
      }
      roh_append(A, rank, first, last, n_het, n_miss);
    };

    uint32_t row = 0, fl = 0;
    meta(0, row, fl);
    PlaneStage g = fetch(0, row, fl);
    meta(1, row, fl);
    for (uint32_t j = 0; j < steps; ++j) {
      uint32_t cal[4], het[4];
      const PlaneFields f(g);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        cal[q] = f.called(q);
        het[q] = (f.b[q] ^ (f.b[q] >> 1)) & cal[q];
      }
      __syncthreads();  // every lane has gathered the step before this one
      s_cal4[tid] = make_uint4(cal[0], cal[1], cal[2], cal[3]);  // tid = srow * 4 + spart
      s_het4[tid] = make_uint4(het[0], het[1], het[2], het[3]);
      __syncthreads();
      if (j + 1 < steps) {  // the next step's loads fly under this step's walk
        g = fetch(j + 1, row, fl);
        meta(j + 2, row, fl);
      }
      if (!active) continue;

      // this lane's bit of the step's 64 rows
      uint64_t hm = 0, mm = 0;
#pragma unroll
      for (uint32_t i = 0; i < kRohStepRows; ++i) {
        const uint32_t c = s_cal[i * 16u + word], h = s_het[i * 16u + word];
        hm |= (uint64_t)((h >> shift) & 1u) << i;
        mm |= (uint64_t)(((c >> shift) & 1u) ^ 1u) << i;
      }

      const uint64_t base = (uint64_t)s + (uint64_t)j * kRohStepRows;
      const uint32_t count = (uint32_t)(end - base < kRohStepRows ? end - base : kRohStepRows);
      // break(d) of the step's decided rows d = base - (W - 1) + i, at bit i
      const uint64_t at = base + 64 - (W - 1);
      const unsigned long long lo = A.brk[at >> 6], up = A.brk[(at >> 6) + 1];
      uint64_t bs = (at & 63) ? (lo >> (at & 63)) | (up << (64 - (at & 63))) : lo;
      for (uint32_t i = 0; i < count; ++i, hm >>= 1, mm >>= 1, bs >>= 1) {
        const uint64_t k = base + i;
        hist_het = (hist_het << 1) | (hm & 1ull);
        hist_miss = (hist_miss << 1) | (mm & 1ull);
        const bool complete = k - s >= W - 1 && k < K;  // window t = k - (W - 1) exists and all its rows were walked
        const bool hom = complete && (uint32_t)__popcll(hist_het & mask_w) <= A.P.window_het && (uint32_t)__popcll(hist_miss & mask_w) <= A.P.window_missing;
        hist_hom = (hist_hom << 1) | (hom ? 1ull : 0ull);
        if (k < (uint64_t)b0 + (W - 1)) continue;
        const uint32_t d = (uint32_t)(k - (W - 1));  // b0 <= d < b1
        const uint32_t t_lo = d + 1 >= W ? d + 1 - W : 0, t_hi = d < K - W ? d : K - W;
        const uint32_t n_cov = t_hi - t_lo + 1;
        const uint32_t need = n_cov == W ? need_full : s_need[n_cov];
        const bool in_run = (uint32_t)__popcll(hist_hom & mask_w) >= need;
        if (open && (!in_run || (bs & 1ull))) close(d - 1);
        if (in_run) {
          if (!open) { open = true; first = d; n_het = n_miss = 0; }
          n_het += (uint32_t)((hist_het >> (W - 1)) & 1ull);
          n_miss += (uint32_t)((hist_miss >> (W - 1)) & 1ull);
        }
      }
    }
    if (active) {
      r32[RohRec::head_last * spad] = head_last; r32[RohRec::head_c * spad] = head_het; r32[(RohRec::head_c + 1) * spad] = head_miss;
      r32[RohRec::tail_first * spad] = open ? first : kSegNone; r32[RohRec::tail_c * spad] = n_het; r32[(RohRec::tail_c + 1) * spad] = n_miss;
      r32[RohRec::runs * spad] = runs; r32[RohRec::sites * spad] = sites;
      r64[0 * spad] = length_sum; r64[1 * spad] = longest;
    }
  }
}

// one thread per selected sample
static __global__ __launch_bounds__(256) void roh_stitch_kernel(const RohArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t nb = A.P.n_bins;
  const size_t spad = (size_t)A.groups * kSegGroupSamples;
  const size_t slot = A.samples ? A.samples[i] : i;
  uint64_t runs = 0, sites = 0, length_sum = 0, longest = 0;
  unsigned long long* bin_runs = A.out.d_bin_runs ? A.out.d_bin_runs + (size_t)i * nb : nullptr;
  unsigned long long* bin_length = A.out.d_bin_length ? A.out.d_bin_length + (size_t)i * nb : nullptr;
  for (uint32_t b = 0; b < nb; ++b) {
    if (bin_runs) bin_runs[b] = 0;
    if (bin_length) bin_length[b] = 0;
  }
  auto judge = [&](uint32_t first, uint32_t last, const uint32_t (&c)[2]) {  // c = (het, miss)
    const uint64_t n_sites = last - first + 1, length = (uint64_t)A.x[last] - A.x[first] + 1;
    if (!roh_qualifies(A.P, n_sites, length, c[0], c[1])) return;
    ++runs; sites += n_sites; length_sum += length; longest = length > longest ? length : longest;
    if (nb) {
      const uint32_t b = roh_bin(A.P, length);
      if (bin_runs) bin_runs[b] += 1;
      if (bin_length) bin_length[b] += length;
    }
    roh_append(A, i, first, last, c[0], c[1]);
  };
  auto interior = [&](uint32_t rb, const uint32_t* r32) {
    const unsigned long long* r64 = A.rec64 + (size_t)rb * (kRohRec64 + 2 * nb) * spad + slot;
    runs += r32[RohRec::runs * spad]; sites += r32[RohRec::sites * spad]; length_sum += r64[0];
    longest = r64[1 * spad] > longest ? r64[1 * spad] : longest;
    for (uint32_t b = 0; b < nb; ++b) {
      if (bin_runs) bin_runs[b] += r64[(kRohRec64 + b) * spad];
      if (bin_length) bin_length[b] += r64[(kRohRec64 + nb + b) * spad];
    }
  };
  seg_stitch<2>(A.rec32 + slot, spad, A.n_blocks, A.item_rows, A.K, A.brk, 64, judge, interior);
  if (A.out.d_n_runs) A.out.d_n_runs[i] = runs;
  if (A.out.d_sum_sites) A.out.d_sum_sites[i] = sites;
  if (A.out.d_sum_length) A.out.d_sum_length[i] = length_sum;
  if (A.out.d_longest_length) A.out.d_longest_length[i] = longest;
}

}  // namespace fmh
