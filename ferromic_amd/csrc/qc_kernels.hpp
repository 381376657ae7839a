// qc_kernels.hpp — gfx950 kernels of the genotype QC (qc.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.17):
// qc_count_kernel (per-site class counts and per-sample class counts in one pass over the bit planes), qc_weighted_kernel (the exact
// per-sample sum of row weights over the rows where the sample is called) and hwe_kernel (the Hardy-Weinberg exact test, one thread per site).
//
// Mapping of the two plane kernels: a lane owns one 32-bit word of the row - 16 diploid samples, sample j of the word at bits 2 j and 2 j + 1 -
// and walks rows.  A workgroup of 256 threads is LW word lanes (a power of two, 8 .. 256, the row's words rounded up) x RL = 256 / LW row
// lanes; a row wider than 256 words is cut into column chunks and a work item is (block of rows, column chunk).  The class words are plain
// integer arithmetic on even bits, as in kin_planes_kernel:
//   called = pc & pc >> 1 & ~(hi | hi >> 1) & selected     het = called & (b0 ^ b0 >> 1)     hom_alt = called & b0 & b0 >> 1
// `selected` is the sample list as a bit mask (bit 2 j per listed sample; zero beyond the row): a list costs no gather.  row_gap / row_hi
// (one byte per row, may be null) spare the called / upper planes of the rows that have nothing there.
//   Site tracks (along the row): popcounts of the class words, packed two to a dword, summed over the word lanes of eight rows at once by a
// transposed butterfly (ten shuffles per eight rows, not forty-eight), gathered per pass in LDS and stored as whole runs of rows.
//   Sample tables (down the columns): bit-sliced vertical counters in registers.  Eight rows go through a carry-save adder tree into the
// slices of weight 1, 2 and 4, the carry of weight 8 ripples into five more; het sits on the even and hom_alt on the odd bits of one
// word, called in a second.  After kQcFlushBlocks blocks (248 rows of a lane, the slices hold 255) and at the end of the item the slices are
// expanded into u32 per-sample counters in LDS, which go to the caller's u64 tables with one 64-bit atomic per sample, table and item.
// Integer adds, exact in any order: the result depends on no grid, item size or route.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_rows.hpp"

namespace fmh {

constexpr uint32_t kQcThreads = 256;
constexpr uint32_t kQcBlockRows = 8;       // rows of a lane per carry-save block
constexpr uint32_t kQcSlices = 8;          // weights 1 .. 128: a lane's slices hold 255
constexpr uint32_t kQcFlushBlocks = 31;    // 31 x 8 = 248 <= 255 rows of a lane between two expansions
constexpr uint32_t kQcMinWordLanes = 8;    // the transposed butterfly hands eight rows to eight lanes
constexpr uint32_t kQcEven = 0x55555555u;

struct QcArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t words;                    // 32-bit words of a row that exist (plane_pitch / 4)
  uint32_t word_lanes;               // LW
  uint32_t n_chunks;                 // column chunks of LW words
  const uint32_t* selected;          // [n_chunks * LW]: bit 2 j of word w = sample 16 w + j is listed
  const uint32_t* rank_before;       // [n_chunks * LW]: listed samples before word w
  size_t row_begin, row_count;
  uint32_t item_rows;
  uint32_t n_items;                  // row blocks x n_chunks; item it = (row block it / n_chunks, chunk it % n_chunks)
  const uint8_t* keep;               // [row_count] or null: the rows the sample tables count
  const uint32_t* weight;            // [row_count] (qc_weighted_kernel)
  unsigned long long weight_total;   // the sum of the kept rows' weights
  uint32_t *site_hom_ref, *site_het, *site_hom_alt;                     // [row_count] each or null
  unsigned long long *hom_ref, *het, *hom_alt, *weighted_called;        // [n] each or null, added into
};

// LDS dwords of qc_count_kernel: two buffers of [8 RL] x 2 track sums, then [3][16 LW] sample counters
__host__ __device__ inline uint32_t qc_track_dwords(uint32_t word_lanes) { return 2u * 2u * kQcBlockRows * (kQcThreads / word_lanes); }
__host__ __device__ inline uint32_t qc_count_lds_dwords(uint32_t word_lanes, bool tables) {
  return qc_track_dwords(word_lanes) + (tables ? 3u * 16u * word_lanes : 0u);
}

// sum, carry of three words
__device__ __forceinline__ void qc_csa(uint32_t a, uint32_t b, uint32_t c, uint32_t& sum, uint32_t& carry) {
  const uint32_t u = a ^ b;
  sum = u ^ c;
  carry = (a & b) | (u & c);
}

// One lane's vertical counter: bit b of s[k] is bit k of the number of rows whose word had bit b.
struct QcSlices {
  uint32_t s[kQcSlices];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (uint32_t k = 0; k < kQcSlices; ++k) s[k] = 0;
  }
  __device__ __forceinline__ void add8(const uint32_t (&v)[kQcBlockRows]) {
    uint32_t twos_a, twos_b, fours_a, fours_b, eights;
    qc_csa(s[0], v[0], v[1], s[0], twos_a);
    qc_csa(s[0], v[2], v[3], s[0], twos_b);
    qc_csa(s[1], twos_a, twos_b, s[1], fours_a);
    qc_csa(s[0], v[4], v[5], s[0], twos_a);
    qc_csa(s[0], v[6], v[7], s[0], twos_b);
    qc_csa(s[1], twos_a, twos_b, s[1], fours_b);
    qc_csa(s[2], fours_a, fours_b, s[2], eights);
#pragma unroll
    for (uint32_t k = 3; k < kQcSlices; ++k) {  // the last carry is zero: the slices are expanded before they hold more than 255
      const uint32_t carry = s[k] & eights;
      s[k] ^= eights;
      eights = carry;
    }
  }
  __device__ __forceinline__ uint32_t count(uint32_t bit) const {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kQcSlices; ++k) c |= ((s[k] >> bit) & 1u) << k;
    return c;
  }
};

// v[i] = this lane's value of row i (i < 8).  Returns the sum over the aligned `width` lanes (8 .. 64, a power of two) of row
// qc_row_of_lane(lane): three exchange steps halve the rows a lane carries while they double the lanes summed, then plain butterflies.
__device__ __forceinline__ uint32_t qc_row_of_lane(uint32_t lane) { return ((lane & 1u) << 2) | (lane & 2u) | ((lane >> 2) & 1u); }
__device__ __forceinline__ uint32_t qc_reduce8(const uint32_t (&v)[kQcBlockRows], uint32_t lane, uint32_t width) {
  uint32_t u[4], w[2];
  const bool b0 = lane & 1u, b1 = lane & 2u, b2 = lane & 4u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t keep = b0 ? v[i + 4] : v[i], give = b0 ? v[i] : v[i + 4];
    u[i] = keep + (uint32_t)__shfl_xor((int)give, 1);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t keep = b1 ? u[i + 2] : u[i], give = b1 ? u[i] : u[i + 2];
    w[i] = keep + (uint32_t)__shfl_xor((int)give, 2);
  }
  uint32_t z = (b2 ? w[1] : w[0]) + (uint32_t)__shfl_xor((int)(b2 ? w[0] : w[1]), 4);
  for (uint32_t m = 8; m < width; m <<= 1) z += (uint32_t)__shfl_xor((int)z, (int)m);
  return z;
}

// The words of one lane's next eight rows as loaded: classified a pass later, so that a pass's loads are in flight while the pass before it is
// counted.  pc is all ones for a row without an uncalled column and ZERO for a row that is not read (past the item, or - with no tracks
// wanted - not kept): such a row classifies to nothing.
struct QcRaw {
  uint32_t b0[kQcBlockRows], pc[kQcBlockRows], hi[kQcBlockRows];
  uint32_t kept;  // bit i: row i counts for the sample tables
};

// Row i of the block is row base + i RL + rl of the item: adjacent row lanes read adjacent rows.  The per-row bytes (keep, row_gap, row_hi) of
// all eight rows are loaded first, from a clamped row so that no load hangs on a branch, then the planes (plane 0 only with P0).
template <bool TRACKS, bool TABLES, bool P0 = true>
__device__ __forceinline__ void qc_load8(const QcArgs& A, size_t first, uint32_t rows, uint32_t base, uint32_t RL, uint32_t rl, uint32_t w,
                                         bool word_live, QcRaw& raw) {
  uint8_t keep[kQcBlockRows], gap[kQcBlockRows], high[kQcBlockRows];
#pragma unroll
  for (uint32_t i = 0; i < kQcBlockRows; ++i) {
    const uint32_t r = base + i * RL + rl, rc = r < rows ? r : rows - 1;
    const size_t row = A.row_begin + first + rc;
    keep[i] = TABLES ? (A.keep ? A.keep[first + rc] : 1) : 0;
    gap[i] = A.pc ? (A.row_gap ? A.row_gap[row] : 1) : 0;
    high[i] = (A.p1 || A.p2) ? (A.row_hi ? A.row_hi[row] : 1) : 0;
  }
  raw.kept = 0;
#pragma unroll
  for (uint32_t i = 0; i < kQcBlockRows; ++i) {
    const uint32_t r = base + i * RL + rl;
    raw.b0[i] = raw.pc[i] = raw.hi[i] = 0;
    if (r < rows && word_live && (TRACKS || keep[i] != 0)) {
      const size_t at = (A.row_begin + first + r) * A.plane_pitch + (size_t)w * 4;
      if (keep[i] != 0) raw.kept |= 1u << i;
      if constexpr (P0) raw.b0[i] = *reinterpret_cast<const uint32_t*>(A.p0 + at);
      raw.pc[i] = gap[i] != 0 ? *reinterpret_cast<const uint32_t*>(A.pc + at) : ~0u;
      if (high[i] != 0) {
        uint32_t hi = A.p1 ? *reinterpret_cast<const uint32_t*>(A.p1 + at) : 0u;
        if (A.p2) hi |= *reinterpret_cast<const uint32_t*>(A.p2 + at);
        raw.hi[i] = hi;
      }
    }
  }
}

// Launched with kQcThreads threads and qc_count_lds_dwords(LW, TABLES) * 4 bytes of dynamic LDS.
template <bool TRACKS, bool TABLES>
__global__ __launch_bounds__(kQcThreads) void qc_count_kernel(const QcArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t qc_lds[];
  const uint32_t LW = A.word_lanes, RL = kQcThreads / LW, pass_rows = kQcBlockRows * RL;
  const uint32_t tid = threadIdx.x, wl = tid % LW, rl = tid / LW;
  uint32_t* s_trk = qc_lds;                        // [2][pass_rows][2]: het | hom_alt << 16, called
  uint32_t* s_cnt = qc_lds + qc_track_dwords(LW);  // [3][16 LW]: het, hom_alt, called of the chunk's samples
  const uint32_t chunk_samples = 16u * LW;
  const uint32_t wave_width = LW < 64u ? LW : 64u;

  for (uint32_t s = tid; s < qc_count_lds_dwords(LW, TABLES); s += kQcThreads) qc_lds[s] = 0;
  __syncthreads();

  uint32_t pass = 0;  // counts on across the items: the two track buffers alternate without a gap
  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t chunk = it % A.n_chunks;
    const size_t first = (size_t)(it / A.n_chunks) * A.item_rows;  // of the range
    const uint32_t rows = (uint32_t)(A.row_count - first < A.item_rows ? A.row_count - first : A.item_rows);
    const uint32_t w = chunk * LW + wl;
    const uint32_t selected = w < A.words ? A.selected[w] : 0u;  // a word without a listed sample is not read
    QcSlices sx, sc;
    sx.clear();
    sc.clear();
    uint32_t blocks = 0;
    auto expand = [&]() {
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) {
        if (!((selected >> (2 * j)) & 1u)) continue;
        const uint32_t het = sx.count(2 * j), alt = sx.count(2 * j + 1), called = sc.count(2 * j);
        if (het) atomicAdd(&s_cnt[wl * 16 + j], het);
        if (alt) atomicAdd(&s_cnt[chunk_samples + wl * 16 + j], alt);
        if (called) atomicAdd(&s_cnt[2 * chunk_samples + wl * 16 + j], called);
      }
      sx.clear();
      sc.clear();
      blocks = 0;
    };

    QcRaw cur, next = {};  // (the last pass copies `next` without having loaded it)
    qc_load8<TRACKS, TABLES>(A, first, rows, 0, RL, rl, w, selected != 0, cur);
    for (uint32_t base = 0; base < rows; base += pass_rows, ++pass) {
      if (base + pass_rows < rows) qc_load8<TRACKS, TABLES>(A, first, rows, base + pass_rows, RL, rl, w, selected != 0, next);
      uint32_t x[kQcBlockRows], cv[kQcBlockRows], ha[kQcBlockRows], cc[kQcBlockRows];
#pragma unroll
      for (uint32_t i = 0; i < kQcBlockRows; ++i) {
        const uint32_t b0 = cur.b0[i], pc = cur.pc[i], hi = cur.hi[i];
        const uint32_t called = selected & pc & (pc >> 1) & ~(hi | (hi >> 1));
        const uint32_t het_alt = (called & (b0 ^ (b0 >> 1))) | ((called & b0 & (b0 >> 1)) << 1);
        if constexpr (TRACKS) {
          ha[i] = (uint32_t)__popc(het_alt & kQcEven) | ((uint32_t)__popc(het_alt & ~kQcEven) << 16);
          cc[i] = (uint32_t)__popc(called);
        }
        const uint32_t kept = (cur.kept >> i) & 1u ? ~0u : 0u;
        x[i] = het_alt & kept;
        cv[i] = called & kept;
      }
      cur = next;
      if constexpr (TABLES) {
        sx.add8(x);
        sc.add8(cv);
        if (++blocks == kQcFlushBlocks) expand();
      }
      if constexpr (TRACKS) {
        // a dword of `ha` sums at most 256 lanes x 16 samples = 4 096 per half: no carry between the halves
        uint32_t* trk = s_trk + (size_t)(pass & 1u) * pass_rows * 2;
        const uint32_t sum_ha = qc_reduce8(ha, wl, wave_width), sum_cc = qc_reduce8(cc, wl, wave_width);
        if ((wl & (wave_width - 1)) < kQcBlockRows) {  // one lane per row and wave: four waves share a row when LW = 256
          const uint32_t q = qc_row_of_lane(wl) * RL + rl;
          if (sum_ha) atomicAdd(&trk[q * 2], sum_ha);
          if (sum_cc) atomicAdd(&trk[q * 2 + 1], sum_cc);
        }
        __syncthreads();
        // pass row q is row base + q of the item.  The buffer of the pass after next is this one: cleared here, added to only behind the
        // next pass's barrier.
        if (tid < pass_rows) {
          const uint32_t sum2 = trk[tid * 2], called = trk[tid * 2 + 1];
          trk[tid * 2] = 0;
          trk[tid * 2 + 1] = 0;
          if (base + tid < rows) {
            const size_t o = first + base + tid;
            const uint32_t het = sum2 & 0xFFFFu, alt = sum2 >> 16, ref = called - het - alt;
            if (A.n_chunks == 1) {  // the only writer of the row: stored
              if (A.site_hom_ref) A.site_hom_ref[o] = ref;
              if (A.site_het) A.site_het[o] = het;
              if (A.site_hom_alt) A.site_hom_alt[o] = alt;
            } else {                // one of n_chunks writers: the tracks were zeroed before the launch
              if (A.site_hom_ref && ref) atomicAdd(&A.site_hom_ref[o], ref);
              if (A.site_het && het) atomicAdd(&A.site_het[o], het);
              if (A.site_hom_alt && alt) atomicAdd(&A.site_hom_alt[o], alt);
            }
          }
        }
      }
    }

    if constexpr (TABLES) {
      if (blocks != 0) expand();
      __syncthreads();
      for (uint32_t i = tid; i < chunk_samples; i += kQcThreads) {
        const uint32_t ww = chunk * LW + i / 16, j = i % 16;
        const uint32_t sel = ww < A.words ? A.selected[ww] : 0u;
        if (!((sel >> (2 * j)) & 1u)) continue;
        const uint32_t rank = A.rank_before[ww] + (uint32_t)__popc(sel & ((1u << (2 * j)) - 1u));
        const uint32_t het = s_cnt[i], alt = s_cnt[chunk_samples + i], called = s_cnt[2 * chunk_samples + i];
        s_cnt[i] = 0;
        s_cnt[chunk_samples + i] = 0;
        s_cnt[2 * chunk_samples + i] = 0;
        const uint32_t ref = called - het - alt;
        if (A.hom_ref && ref) atomicAdd(&A.hom_ref[rank], (unsigned long long)ref);
        if (A.het && het) atomicAdd(&A.het[rank], (unsigned long long)het);
        if (A.hom_alt && alt) atomicAdd(&A.hom_alt[rank], (unsigned long long)alt);
      }
      __syncthreads();
    }
  }
}

// sum over the kept rows of w_r c_s(r) = (sum over the kept rows of w_r) - sum of w_r over the kept rows where s is NOT called: only the set
// bits of the uncalled word are visited, a row without an uncalled column and without an upper allele is not read at all, and plane 0 never;
// eight rows of a lane are loaded at once (qc_load8).
// The item with row block 0 adds the total; every item subtracts what it found (two's complement: exact modulo 2^64, and the true sum is
// non-negative).  Launched with kQcThreads threads and 16 LW x 8 bytes of dynamic LDS.
__global__ __launch_bounds__(kQcThreads) void qc_weighted_kernel(const QcArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long qc_wlds[];
  const uint32_t LW = A.word_lanes, RL = kQcThreads / LW;
  const uint32_t tid = threadIdx.x, wl = tid % LW, rl = tid / LW;
  const uint32_t chunk_samples = 16u * LW;
  for (uint32_t s = tid; s < chunk_samples; s += kQcThreads) qc_wlds[s] = 0;
  __syncthreads();

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t chunk = it % A.n_chunks;
    const size_t first = (size_t)(it / A.n_chunks) * A.item_rows;
    const uint32_t rows = (uint32_t)(A.row_count - first < A.item_rows ? A.row_count - first : A.item_rows);
    const uint32_t w = chunk * LW + wl;
    const uint32_t selected = w < A.words ? A.selected[w] : 0u;
    if (selected != 0) {
      for (uint32_t base = 0; base < rows; base += kQcBlockRows * RL) {
        uint32_t weight[kQcBlockRows];
#pragma unroll
        for (uint32_t i = 0; i < kQcBlockRows; ++i) {
          const uint32_t r = base + i * RL + rl;
          weight[i] = A.weight[first + (r < rows ? r : rows - 1)];
        }
        QcRaw raw;
        qc_load8<false, true, false>(A, first, rows, base, RL, rl, w, true, raw);
#pragma unroll
        for (uint32_t i = 0; i < kQcBlockRows; ++i) {
          const uint32_t pc = raw.pc[i], hi = raw.hi[i];
          const uint32_t called = selected & pc & (pc >> 1) & ~(hi | (hi >> 1));
          if (!((raw.kept >> i) & 1u) || weight[i] == 0) continue;  // (a row that is not kept was not read: its pc is zero)
          for (uint32_t u = selected & ~called; u != 0; u &= u - 1)
            atomicAdd(&qc_wlds[wl * 16 + ((uint32_t)__ffs((int)u) - 1u) / 2], (unsigned long long)weight[i]);
        }
      }
    }
    __syncthreads();
    const unsigned long long total = it / A.n_chunks == 0 ? A.weight_total : 0ull;
    for (uint32_t i = tid; i < chunk_samples; i += kQcThreads) {
      const uint32_t ww = chunk * LW + i / 16, j = i % 16;
      const uint32_t sel = ww < A.words ? A.selected[ww] : 0u;
      if (!((sel >> (2 * j)) & 1u)) continue;
      const uint32_t rank = A.rank_before[ww] + (uint32_t)__popc(sel & ((1u << (2 * j)) - 1u));
      const unsigned long long add = total - qc_wlds[i];
      qc_wlds[i] = 0;
      if (add) atomicAdd(&A.weighted_called[rank], add);
    }
    __syncthreads();
  }
}

// ---- the Hardy-Weinberg exact test (Wigginton, Cutler & Abecasis 2005), array-free: the DEFINITION is include/ferromic_hip.h's ------------
constexpr uint64_t kHweMaxGenotypes = (uint64_t)1 << 26;  // the integer products stay below 2^53

// One walk over the het counts of the site's parity, in the order mid, down, up, of weights relative to the one at `mid`.
// SECOND = false: returns the sum of all weights, *t_obs = the weight at x == het.  SECOND = true: returns the sum of the weights <= *t_obs.
template <bool SECOND>
__host__ __device__ inline double hwe_walk(uint64_t N, uint64_t rare, uint64_t mid, uint64_t het, double* t_obs) {
  const double limit = *t_obs;
  double sum = 0.0, at_het = 0.0;
  auto term = [&](uint64_t x, double t) {
    if constexpr (SECOND) { if (t <= limit) sum += t; }
    else { sum += t; if (x == het) at_het = t; }
  };
  term(mid, 1.0);
  double t = 1.0;
  uint64_t x = mid, r = (rare - mid) / 2, c = N - x - r;
  while (x >= 2) {
    t = (t * (double)(x * (x - 1))) / (double)(4 * (r + 1) * (c + 1));
    x -= 2; ++r; ++c;
    if (t == 0.0) break;  // every later term is zero too
    term(x, t);
  }
  t = 1.0;
  x = mid; r = (rare - mid) / 2; c = N - x - r;
  while (x + 2 <= rare) {
    t = (t * (double)(4 * r * c)) / (double)((x + 2) * (x + 1));
    x += 2; --r; --c;
    if (t == 0.0) break;
    term(x, t);
  }
  if constexpr (!SECOND) *t_obs = at_het;
  return sum;
}

__host__ __device__ inline double hwe_exact_p(uint32_t hom_ref, uint32_t het, uint32_t hom_alt) {
  const uint64_t N = (uint64_t)het + hom_ref + hom_alt;
  if (N == 0 || N > kHweMaxGenotypes) return __builtin_nan("");
  const uint64_t rare = 2 * (uint64_t)(hom_ref < hom_alt ? hom_ref : hom_alt) + het, common = 2 * N - rare;
  if (rare == 0) return 1.0;
  uint64_t mid = rare * common / (2 * N);
  if ((mid ^ rare) & 1) ++mid;
  double t_obs = 0.0;
  const double S = hwe_walk<false>(N, rare, mid, het, &t_obs);
  const double P = hwe_walk<true>(N, rare, mid, het, &t_obs);
  const double p = P / S;
  return p > 1.0 ? 1.0 : p;
}

__global__ __launch_bounds__(256) void hwe_kernel(const uint32_t* __restrict__ hom_ref, const uint32_t* __restrict__ het,
                                                  const uint32_t* __restrict__ hom_alt, size_t n_sites, double* __restrict__ p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_sites) p[i] = hwe_exact_p(hom_ref[i], het[i], hom_alt[i]);
}

}  // namespace fmh
