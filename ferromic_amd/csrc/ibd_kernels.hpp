// ibd_kernels.hpp — gfx950 kernels of the IBD segments (ibd.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.22).
// The second statistic here whose work is a stateful scan ALONG rows (after roh_kernels.hpp), and the first with a state machine per PAIR
// of samples: n (n - 1) / 2 of them.
//
// States (ibd_states_kernel).  For the selected samples and the kept rows it builds the sample-major bit image T[plane][w][sample]: u64
// words, the sample's LIST POSITION fastest and padded to the pair tile, word w = kept rows 64 w .. 64 w + 63; planes R (called, dosage 0),
// A (called, dosage 2) and - for a matrix with a called or an upper plane - C (called).  Bits of rows >= K are zero in every plane, and so
// are the words of the padding samples (the host zeroes T first).  The fetch is the ROH scan's (segment_kernels.hpp: plane_fetch): an
// item = (word w, group of 256 matrix samples); through the kept-row list, 16 bytes per thread and plane (thread = row of the word x
// 16-byte part of the group's 64 bytes; upper planes, row_gap / row_hi honoured through the per-kept-row flags of plane_flags_kernel),
// 2-bit fields parked in LDS; a lane then gathers ITS sample's bit of the 64 rows.
// Pairs (ibd_pair_kernel<MODE, CALLED>).  An item on the persistent grid = (block of item_rows kept rows [b0, b1), b0 a multiple of 64;
// tile pair ti <= tj of 32 x 32 samples).  256 threads; thread (ty, tx) owns the 2 x 2 pairs i = 32 ti + 2 ty + {0, 1},
// j = 32 tj + 2 tx + {0, 1}: every loaded sample word serves two pairs and every per-pair array is indexed by constants after unrolling.
// The tile's 64 samples x planes x a batch of kIbdBatch words are staged in LDS; the next batch's loads are issued before the walk of the
// current one.  Per pair and word: D (discordant rows) = (Ri & Aj) | (Ai & Rj) for IBD1, Ci & Cj & ((Ri ^ Rj) | (Ai ^ Aj)) for IBD2;
// M (missing rows) = valid & ~(Ci & Cj); B (break bits) is the same for all pairs.  A word with D | B == 0 extends (or opens) the pair's
// run and adds popcount(M); otherwise the events are walked lowest first.  Runs strictly inside the block are judged, tallied and (when
// asked for) appended by the lane itself; per (block, pair) the item leaves the record of segment_kernels.hpp (SegRec<1>: head, tail and
// the interior tallies).  A record field is [block][field][slot], slot = 1024 tile + 256 sub-pair + thread: a wave's stores are contiguous.
// Stitch (ibd_stitch_kernel).  One thread per slot joins the blocks by the shared rule (seg_stitch), judges the joined runs, adds the
// interior tallies and writes BOTH triangles of the
// tables (the threads of the slots with i == j write the diagonal's zeros): one writer per entry, nothing is zeroed, no atomics touch the
// tables.  Segments are appended with a vector atomicAdd on a device counter, stored below the capacity (seg_append).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ferromic_hip.h"
#include "plane_rows.hpp"
#include "segment_kernels.hpp"

namespace fmh {

constexpr uint32_t kIbdThreads = 256;
constexpr uint32_t kIbdTile = 32;            // samples of a pair tile's side
constexpr uint32_t kIbdTileSlots = 1024;     // pairs of a tile pair: 256 threads x (2 x 2)
constexpr uint32_t kIbdBatch = 8;            // words of a sample staged in LDS at a time
using IbdRec = SegRec<1>;                    // a run carries (miss)
constexpr size_t kIbdRecBytes = IbdRec::n32 * sizeof(uint32_t) + kSegRec64 * sizeof(unsigned long long);  // per (block, slot)

struct IbdStateArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t nvec;    // 16-byte vectors of a row through the last selected sample (<= plane_pitch / 16)
  uint32_t groups;  // sample groups: ceil(nvec / 4)
  size_t row_begin;
  const uint32_t* rows;   // [K] kept rows, relative to row_begin
  const uint8_t* flags;   // [K] bit 0: the called plane of the row is read, bit 1: the upper planes are; null = neither exists
  const uint32_t* rank;   // [groups * 256] list position of a matrix sample, kSegNone where it is not selected
  uint32_t K, words;      // words = ceil(K / 64)
  uint32_t n_planes;      // 2 (R, A) or 3 (R, A, C)
  uint64_t n_items;       // words * groups
  size_t spad;            // samples of T: n padded to the tile
  unsigned long long* T;  // [n_planes][words][spad]
};

struct IbdArgs {
  const unsigned long long* T;     // [planes][words][spad]
  size_t spad;
  uint32_t words;
  const uint32_t* rows;            // [K] kept rows, relative to row_begin
  const uint32_t* x;               // [K] positions of the kept rows
  const unsigned long long* brk;   // [words] break(k) at bit k & 63 of word k >> 6
  uint32_t n, K, item_rows, n_blocks;
  uint32_t n_tiles;                // tile pairs ti <= tj: t (t + 1) / 2 for t = spad / 32
  uint32_t n_items;                // n_blocks * n_tiles
  fmh_ibd_params P;
  uint32_t* rec32;                 // [n_blocks][IbdRec::n32][n_tiles * 1024]
  unsigned long long* rec64;       // [n_blocks][kSegRec64][n_tiles * 1024]
  fmh_ibd_segment* segments;       // device, `capacity` elements, or null
  unsigned long long capacity;
  unsigned long long* counter;     // null = segments are neither counted nor stored
  fmh_ibd_out out;
};

__device__ __forceinline__ void ibd_append(const IbdArgs& A, uint32_t a, uint32_t b, uint32_t first, uint32_t last, uint32_t n_missing) {
  seg_append(A, [&] { return fmh_ibd_segment{a, b, last - first + 1, n_missing, A.rows[first], A.rows[last]}; });
}
// tile pair t = tj (tj + 1) / 2 + ti, ti <= tj
__device__ __forceinline__ void ibd_tile_of(uint32_t t, uint32_t& ti, uint32_t& tj) {
  uint64_t c = (uint64_t)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (c * (c + 1) / 2 > t) --c;
  while ((c + 1) * (c + 2) / 2 <= t) ++c;
  tj = (uint32_t)c;
  ti = t - (uint32_t)(c * (c + 1) / 2);
}

// Launched with kIbdThreads threads; static LDS: 3 x 4 KiB of fields.
static __global__ __launch_bounds__(kIbdThreads) void ibd_states_kernel(const IbdStateArgs A) {
  __shared__ uint4 s_ref4[64 * 4];  // [row of the word][16-byte part]: a row's 16 words of 2-bit fields
  __shared__ uint4 s_alt4[64 * 4];
  __shared__ uint4 s_cal4[64 * 4];
  const uint32_t* s_ref = reinterpret_cast<const uint32_t*>(s_ref4);
  const uint32_t* s_alt = reinterpret_cast<const uint32_t*>(s_alt4);
  const uint32_t* s_cal = reinterpret_cast<const uint32_t*>(s_cal4);
  const uint32_t tid = threadIdx.x;
  const uint32_t srow = tid >> 2, spart = tid & 3u;          // the staging thread's row of the word and 16-byte part of the group's 64 bytes
  const uint32_t word = tid >> 4, shift = 2u * (tid & 15u);  // the gathering lane's word of a row's 16 and its field in it
  const size_t plane_words = (size_t)A.words * A.spad;
  for (uint64_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t w = (uint32_t)(it / A.groups), sg = (uint32_t)(it % A.groups);
    const uint64_t k = (uint64_t)w * 64 + srow;
    const uint32_t kk = k < A.K ? (uint32_t)k : A.K - 1;
    const uint32_t row = A.rows[kk], fl = A.flags ? (uint32_t)A.flags[kk] : 0u;
    const uint32_t vec = 4u * sg + spart;
    const bool inside = vec < A.nvec;  // a vector past the covered samples is zero
    const bool ok = inside && k < A.K;
    const size_t off = (A.row_begin + row) * A.plane_pitch + (size_t)(inside ? vec : 0) * 16;
    const PlaneFields f(plane_fetch(A, off, ok, fl));
    uint32_t cal[4], ref[4], alt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cal[q] = f.called(q);
      ref[q] = cal[q] & ~(f.b[q] | (f.b[q] >> 1));
      alt[q] = cal[q] & f.b[q] & (f.b[q] >> 1);
    }
    __syncthreads();  // every lane has gathered the item before this one
    s_ref4[tid] = make_uint4(ref[0], ref[1], ref[2], ref[3]);  // tid = srow * 4 + spart
    s_alt4[tid] = make_uint4(alt[0], alt[1], alt[2], alt[3]);
    s_cal4[tid] = make_uint4(cal[0], cal[1], cal[2], cal[3]);
    __syncthreads();
    const uint32_t rank = A.rank[(size_t)sg * kSegGroupSamples + tid];
    if (rank == kSegNone) continue;
    uint64_t rm = 0, am = 0, cm = 0;
#pragma unroll
    for (uint32_t i = 0; i < 64; ++i) {
      rm |= (uint64_t)((s_ref[i * 16u + word] >> shift) & 1u) << i;
      am |= (uint64_t)((s_alt[i * 16u + word] >> shift) & 1u) << i;
      cm |= (uint64_t)((s_cal[i * 16u + word] >> shift) & 1u) << i;
    }
    unsigned long long* t = A.T + (size_t)w * A.spad + rank;
    t[0] = rm;
    t[plane_words] = am;
    if (A.n_planes == 3) t[2 * plane_words] = cm;
  }
}

// Launched with kIbdThreads threads; static LDS: planes x kIbdBatch x 64 words (8 or 12 KiB).
template <uint32_t MODE, bool CALLED>
static __global__ __launch_bounds__(kIbdThreads) void ibd_pair_kernel(const IbdArgs A) {
  constexpr uint32_t NP = CALLED ? 3 : 2;
  constexpr uint32_t kLoads = NP * kIbdBatch * 64 / kIbdThreads;  // words a thread stages per batch: 2 per plane
  __shared__ ulonglong2 s_t2[NP * kIbdBatch * 32];                // [plane][word of the batch][i half: 32 samples, j half: 32 samples]
  unsigned long long* s_t = reinterpret_cast<unsigned long long*>(s_t2);
  const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15u;
  const size_t plane_words = (size_t)A.words * A.spad;
  const size_t slots = (size_t)A.n_tiles * kIbdTileSlots;
  const uint32_t K = A.K;

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t rb = it / A.n_tiles, tp = it % A.n_tiles;
    uint32_t ti, tj;
    ibd_tile_of(tp, ti, tj);
    const uint32_t b0 = rb * A.item_rows, b1 = K - b0 < A.item_rows ? K : b0 + A.item_rows;
    const uint32_t w0 = b0 >> 6, nw = (b1 - b0 + 63) >> 6;
    const uint32_t batches = (nw + kIbdBatch - 1) / kIbdBatch;
    const uint32_t i0 = ti * kIbdTile + 2 * ty, j0 = tj * kIbdTile + 2 * tx;
    bool active[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) active[q] = i0 + (q >> 1) < j0 + (q & 1u) && j0 + (q & 1u) < A.n;

    // element e of a thread's batch share: flat LDS index e * 256 + tid = plane * 512 + word * 64 + half * 32 + sample
    const uint32_t l_sample = ((tid >> 5) & 1u ? tj : ti) * kIbdTile + (tid & 31u), l_word = tid >> 6;
    auto fetch = [&](uint32_t batch, unsigned long long (&g)[kLoads]) {
#pragma unroll
      for (uint32_t e = 0; e < kLoads; ++e) {
        const uint32_t plane = e >> 1, s = ((e & 1u) << 2) | l_word;
        const uint32_t w = batch * kIbdBatch + s;
        g[e] = w < nw ? A.T[plane * plane_words + (size_t)(w0 + w) * A.spad + l_sample] : 0ull;
      }
    };

    // the four pairs' scan state
    uint32_t first[4], miss[4], head_last[4], head_miss[4], runs[4], sites[4];
    uint64_t length_sum[4], longest[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      first[q] = head_last[q] = kSegNone;
      miss[q] = head_miss[q] = runs[q] = sites[q] = 0;
      length_sum[q] = longest[q] = 0;
    }

    unsigned long long g[kLoads];
    fetch(0, g);
    for (uint32_t batch = 0; batch < batches; ++batch) {
      __syncthreads();  // every lane has walked the batch before this one
#pragma unroll
      for (uint32_t e = 0; e < kLoads; ++e) s_t[e * kIbdThreads + tid] = g[e];
      __syncthreads();
      if (batch + 1 < batches) fetch(batch + 1, g);  // the next batch's loads fly under this batch's walk
      const uint32_t left = nw - batch * kIbdBatch, steps = left < kIbdBatch ? left : kIbdBatch;
      for (uint32_t s = 0; s < steps; ++s) {
        const uint32_t wi = w0 + batch * kIbdBatch + s;
        const uint32_t base = wi << 6;
        const uint32_t cnt = b1 - base < 64u ? b1 - base : 64u;
        const uint64_t valid = cnt == 64u ? ~0ull : ((1ull << cnt) - 1ull);
        const uint64_t B = A.brk[wi];
        const ulonglong2 ri = s_t2[(0 * kIbdBatch + s) * 32 + ty], rj = s_t2[(0 * kIbdBatch + s) * 32 + 16 + tx];
        const ulonglong2 ai = s_t2[(1 * kIbdBatch + s) * 32 + ty], aj = s_t2[(1 * kIbdBatch + s) * 32 + 16 + tx];
        ulonglong2 ci = make_ulonglong2(0, 0), cj = ci;
        if (CALLED) {
          ci = s_t2[(2 * kIbdBatch + s) * 32 + ty];
          cj = s_t2[(2 * kIbdBatch + s) * 32 + 16 + tx];
        }
        const uint64_t Ri[2] = {ri.x, ri.y}, Rj[2] = {rj.x, rj.y}, Ai[2] = {ai.x, ai.y}, Aj[2] = {aj.x, aj.y};
        const uint64_t Ci[2] = {ci.x, ci.y}, Cj[2] = {cj.x, cj.y};
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          if (!active[q]) continue;
          const uint32_t qi = q >> 1, qj = q & 1u;
          const uint64_t both = CALLED ? (Ci[qi] & Cj[qj]) : ~0ull;
          const uint64_t D = MODE == FMH_IBD1 ? ((Ri[qi] & Aj[qj]) | (Ai[qi] & Rj[qj])) : (both & ((Ri[qi] ^ Rj[qj]) | (Ai[qi] ^ Aj[qj])));
          const uint64_t M = CALLED ? (valid & ~both) : 0ull;
          // a run [f, last] has ended: the block's head goes to the stitch, an interior run is judged here
          auto close = [&](uint32_t last) {
            const uint32_t f = first[q];
            first[q] = kSegNone;
            if (f == b0) {
              head_last[q] = last; head_miss[q] = miss[q];
              return;
            }
            const uint32_t n_sites = last - f + 1;
            if (n_sites < A.P.min_sites || miss[q] > A.P.max_missing) return;  // before the positions are fetched
            const uint64_t length = (uint64_t)A.x[last] - A.x[f] + 1;
            if (!run_qualifies(A.P, n_sites, length, miss[q])) return;
            ++runs[q]; sites[q] += n_sites; length_sum[q] += length; longest[q] = length > longest[q] ? length : longest[q];
            ibd_append(A, i0 + qi, j0 + qj, f, last, miss[q]);
          };
          uint64_t events = D | B;  // rows >= K hold neither a D nor a B bit
          if (events == 0) {
            if (first[q] == kSegNone) { first[q] = base; miss[q] = 0; }
            miss[q] += (uint32_t)__popcll(M);
            continue;
          }
          uint32_t pos = 0;  // the first row of the word not yet accounted for; <= 63 inside the loop
          do {
            const uint32_t e = (uint32_t)__builtin_ctzll(events);
            events &= events - 1;
            if (e > pos && first[q] == kSegNone) { first[q] = base + pos; miss[q] = 0; }
            if (first[q] != kSegNone) {
              miss[q] += (uint32_t)__popcll(M & ((1ull << e) - 1ull) & ~((1ull << pos) - 1ull));
              close(base + e - 1);
            }
            pos = e + (uint32_t)((D >> e) & 1ull);  // a DISC row is in no run; a row behind a break opens the next
          } while (events);
          if (pos < cnt) { first[q] = base + pos; miss[q] = (uint32_t)__popcll(M >> pos); }
        }
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (!active[q]) continue;
      const size_t slot = (size_t)tp * kIbdTileSlots + q * kIbdThreads + tid;
      uint32_t* r32 = A.rec32 + (size_t)rb * IbdRec::n32 * slots + slot;
      unsigned long long* r64 = A.rec64 + (size_t)rb * kSegRec64 * slots + slot;
      r32[IbdRec::head_last * slots] = head_last[q]; r32[IbdRec::head_c * slots] = head_miss[q];
      r32[IbdRec::tail_first * slots] = first[q]; r32[IbdRec::tail_c * slots] = miss[q];
      r32[IbdRec::runs * slots] = runs[q]; r32[IbdRec::sites * slots] = sites[q];
      r64[0 * slots] = length_sum[q]; r64[1 * slots] = longest[q];
    }
  }
}

// one thread per slot (tile pair, sub-pair, thread of the pair kernel)
static __global__ __launch_bounds__(256) void ibd_stitch_kernel(const IbdArgs A) {
  const size_t slots = (size_t)A.n_tiles * kIbdTileSlots;
  const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= slots) return;
  const uint32_t tp = (uint32_t)(slot / kIbdTileSlots), q = (uint32_t)(slot / kIbdThreads) & 3u, tid = (uint32_t)slot & (kIbdThreads - 1);
  uint32_t ti, tj;
  ibd_tile_of(tp, ti, tj);
  const uint32_t i = ti * kIbdTile + 2 * (tid >> 4) + (q >> 1), j = tj * kIbdTile + 2 * (tid & 15u) + (q & 1u);
  const size_t n = A.n;
  if (i == j && i < n) {  // the diagonal: one slot of a diagonal tile per sample
    if (A.out.d_n_segments) A.out.d_n_segments[i * n + i] = 0;
    if (A.out.d_sum_sites) A.out.d_sum_sites[i * n + i] = 0;
    if (A.out.d_sum_length) A.out.d_sum_length[i * n + i] = 0;
    if (A.out.d_longest_length) A.out.d_longest_length[i * n + i] = 0;
  }
  if (!(i < j && j < n)) return;
  uint64_t runs = 0, sites = 0, length_sum = 0, longest = 0;
  auto judge = [&](uint32_t first, uint32_t last, const uint32_t (&c)[1]) {  // c = (miss)
    const uint64_t n_sites = last - first + 1, length = (uint64_t)A.x[last] - A.x[first] + 1;
    if (!run_qualifies(A.P, n_sites, length, c[0])) return;
    ++runs; sites += n_sites; length_sum += length; longest = length > longest ? length : longest;
    ibd_append(A, i, j, first, last, c[0]);
  };
  auto interior = [&](uint32_t rb, const uint32_t* r32) {
    const unsigned long long* r64 = A.rec64 + (size_t)rb * kSegRec64 * slots + slot;
    runs += r32[IbdRec::runs * slots]; sites += r32[IbdRec::sites * slots]; length_sum += r64[0];
    longest = r64[1 * slots] > longest ? r64[1 * slots] : longest;
  };
  seg_stitch<1>(A.rec32 + slot, slots, A.n_blocks, A.item_rows, A.K, A.brk, 0, judge, interior);
  const size_t ij = (size_t)i * n + j, ji = (size_t)j * n + i;
  if (A.out.d_n_segments) A.out.d_n_segments[ij] = A.out.d_n_segments[ji] = runs;
  if (A.out.d_sum_sites) A.out.d_sum_sites[ij] = A.out.d_sum_sites[ji] = sites;
  if (A.out.d_sum_length) A.out.d_sum_length[ij] = A.out.d_sum_length[ji] = length_sum;
  if (A.out.d_longest_length) A.out.d_longest_length[ij] = A.out.d_longest_length[ji] = longest;
}

}  // namespace fmh
