// ehh_kernels.hpp — extended haplotype homozygosity scans from the packed bit planes: per (focal row, side) the pair counts of the two core
// classes after every flanking row, folded by the stop rules into one integer record (ehh.hip; definition in include/ferromic_hip.h, scheme
// and measurements in DESIGN.md section 3.14).
//
// One workgroup owns one item (focal, side); a persistent grid walks the items by block stride.  The partition refinement is that of
// hap_kernels.hpp - the same LDS layout (hap_lds_bytes), the same mark / scan / relabel step per plane, the parked row state, the member
// column table and the next-row line fetch - with four differences:
//   start    the focal row gives the core of every member (0 = called allele 0, 1 = called allele 1, neither otherwise); the cores are counted
//            over the workgroup, core 0 starts as class 0 and core 1 as the class after it.  A member of neither core gets the label 0xFFFF
//            (no class: labels are below n < 0xFFFF) and every later pass over the members skips it before it reads anything.
//   boundary dense ranks are monotone in the key, so the classes of core 0 stay below those of core 1 through every relabel; B = the number of
//            core-0 classes becomes the rank of key 2 B (a prefix plus a popcount, one uniform LDS read).
//   recount  after a row in which K changed, the class sizes go into the free high halves (LDS atomic add, as the end of a window does, but
//            one add per wave for each of the first classes a wave meets), sum c (c - 1) / 2 is folded per core over the K classes and
//            reduced over the workgroup.  A row without a split costs no recount.
//   stop     every thread holds the same counts and runs the stop rules on them (no divergence, nothing to broadcast); thread 0 stores.
// The descending side walks rows downward, and the line fetch follows it.  Outputs leave with plain stores: nothing else writes an item's
// record or its slice of the curve.
#pragma once

#include "hap_kernels.hpp"

namespace fmh {

// the record of include/ferromic_hip.h's fmh_ehh_side
struct EhhSide {
  unsigned long long area2[2], pair_steps[2];
  uint32_t steps[2], core[2], flags, reserved;
};

constexpr uint32_t kEhhEdge0 = 1u, kEhhGap0 = 4u, kEhhSkipped = 16u;  // FMH_EHH_EDGE0 (<< core), FMH_EHH_GAP0 (<< core), FMH_EHH_SKIPPED
constexpr uint32_t kEhhNoClass = 0xFFFFu;
constexpr uint32_t kEhhMaxMembers = kHapMaxMembers;  // the same 4.75 bytes per member: the scan adds no LDS
static_assert(kEhhMaxMembers < kEhhNoClass, "the label of a member of neither core is no class");

struct EhhArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  const uint32_t* cols;              // [n]: the column of member rank r, ascending
  uint32_t n;
  uint32_t touch_first, touch_last;  // byte offsets of the first and last plane dword of a row that holds a member
  const unsigned long long* focal;   // [n_items / 2]
  unsigned long long n_items;        // item i = focal i / 2, side i % 2 (0 = left, rows descend)
  unsigned long long row_begin, row_end;
  const uint32_t* pos;               // [row_end - row_begin]: x of the rows of the range, or null (x(r) = r)
  uint32_t num, den, max_extent, max_gap, min_core;
  EhhSide* out;                      // [n_items]
  uint32_t* pairs;                   // [n_items][2][max_extent] or null
};

// the state of member column c at a row: bits 0..2 = allele bits under the called plane, bit 3 = called; 0 = uncalled
template <int PLANES, bool CALLED>
__device__ __forceinline__ uint32_t ehh_state(const EhhArgs& A, size_t row_off, uint32_t c, bool read_called, bool read_p1, bool read_p2) {
  const size_t at = row_off + (size_t)(c >> 5) * 4;
  const uint32_t sh = c & 31u;
  uint32_t called = 1u;
  if (CALLED && read_called) called = (*reinterpret_cast<const uint32_t*>(A.pc + at) >> sh) & 1u;
  uint32_t bits = (*reinterpret_cast<const uint32_t*>(A.p0 + at) >> sh) & 1u;
  if (PLANES >= 2 && read_p1) bits |= ((*reinterpret_cast<const uint32_t*>(A.p1 + at) >> sh) & 1u) << 1;
  if (PLANES >= 3 && read_p2) bits |= ((*reinterpret_cast<const uint32_t*>(A.p2 + at) >> sh) & 1u) << 2;
  return called ? (bits | 8u) : 0u;
}

// Launched with 64, 256, 512 or 1 024 threads and hap_lds_bytes(n) of dynamic LDS; PLANES / CALLED as hap_kernel.
template <int PLANES, bool CALLED>
__global__ __launch_bounds__(1024) void ehh_kernel(const EhhArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ehh_lds[];
  const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = T >> 6;
  const uint32_t log2_T = 31u - (uint32_t)__clz((int)T);  // T is a power of two
  const uint32_t n = A.n, nw = hap_bitmap_words(n);
  uint32_t* s_wsum = ehh_lds;
  uint32_t* s_red = ehh_lds + 16;  // [16 waves][2]: the cores' counts at the focal row, then their pair counts
  uint32_t* label = ehh_lds + kHapLdsHead;  // [n]: low half = the member's label, high half = parked row state / class size
  uint32_t* bitmap0 = label + hap_pad4(n);
  uint32_t* bitmap1 = bitmap0 + nw;
  uint32_t* prefix = bitmap1 + nw;
  const uint32_t touch_at = A.touch_first + tid * 128u;

  for (unsigned long long item = blockIdx.x; item < A.n_items; item += gridDim.x) {
    const unsigned long long f = A.focal[item >> 1];
    const bool up = (item & 1u) != 0;
    __syncthreads();  // the previous item's last reads of label[] and s_red[]

    // ---- the focal row: the core of every member, the cores' sizes
    uint32_t c0 = 0, c1 = 0;
    {
      const bool read_called = CALLED && (!A.row_gap || A.row_gap[f] != 0);
      const bool read_p1 = PLANES >= 2 && (!A.row_hi || A.row_hi[f] != 0), read_p2 = PLANES >= 3 && read_p1;
      const size_t row_off = (size_t)f * A.plane_pitch;
      for (uint32_t r = tid; r < n; r += T) {
        const uint32_t bits = ehh_state<PLANES, CALLED>(A, row_off, A.cols[r], read_called, read_p1, read_p2);
        const uint32_t core = bits == 8u ? 0u : bits == 9u ? 1u : 2u;
        label[r] = core;
        c0 += core == 0u;
        c1 += core == 1u;
      }
    }
    for (uint32_t i = tid; i < 2 * nw; i += T) bitmap0[i] = 0;  // both bitmaps
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c0 += __shfl_xor(c0, o);
      c1 += __shfl_xor(c1, o);
    }
    if (lane == 0) {
      s_red[2 * wave] = c0;
      s_red[2 * wave + 1] = c1;
    }
    __syncthreads();
    uint32_t n0 = 0, n1 = 0;
    for (uint32_t v = 0; v < waves; ++v) {
      n0 += s_red[2 * v];
      n1 += s_red[2 * v + 1];
    }
    uint32_t B = n0 ? 1u : 0u;          // classes of core 0: labels [0, B); those of core 1: [B, K)
    uint32_t K = B + (n1 ? 1u : 0u);
    const uint32_t n_act = n0 + n1;
    for (uint32_t r = tid; r < n; r += T) {  // the thread's own words
      const uint32_t core = label[r];
      label[r] = core == 0u ? 0u : core == 1u ? B : kEhhNoClass;
    }

    // ---- the stop rules' state: the same in every thread
    const unsigned long long P_init0 = (unsigned long long)n0 * (n0 - (n0 ? 1u : 0u)) / 2, P_init1 = (unsigned long long)n1 * (n1 - (n1 ? 1u : 0u)) / 2;
    const bool skipped = min(n0, n1) < A.min_core;
    uint32_t alive = skipped ? 0u : (P_init0 ? 1u : 0u) | (P_init1 ? 2u : 0u);
    alive = __builtin_amdgcn_readfirstlane(alive);
    unsigned long long P0 = P_init0, P1 = P_init1, prev0 = P_init0, prev1 = P_init1;
    unsigned long long area0 = 0, area1 = 0, psteps0 = 0, psteps1 = 0;
    uint32_t steps0 = 0, steps1 = 0, flags = skipped ? kEhhSkipped : 0u;
    uint32_t* curve = A.pairs ? A.pairs + (size_t)item * 2 * A.max_extent : nullptr;

    unsigned long long limit = up ? A.row_end - 1 - f : f - A.row_begin;
    if (A.max_extent && limit > A.max_extent) limit = A.max_extent;
    uint32_t x_prev = A.pos ? A.pos[f - A.row_begin] : 0u;
    uint32_t cur = 0, dirty_words = 0;

    for (unsigned long long d = 1; d <= limit && alive; ++d) {
      const size_t row = up ? (size_t)(f + d) : (size_t)(f - d);
      uint32_t gap = 1u;
      if (A.pos) {
        const uint32_t x = A.pos[row - A.row_begin];
        gap = x > x_prev ? x - x_prev : x_prev - x;
        x_prev = x;
      }
      if (A.max_gap && gap > A.max_gap) {  // rule 1: every core still alive meets the same gap
        flags |= alive * kEhhGap0;
        alive = 0;
        break;
      }

      const bool read_called = CALLED && (!A.row_gap || A.row_gap[row] != 0);
      const bool read_p1 = PLANES >= 2 && (!A.row_hi || A.row_hi[row] != 0), read_p2 = PLANES >= 3 && read_p1;
      const uint32_t steps = 1u | (read_p1 ? 2u : 0u) | (read_p2 ? 4u : 0u) | (read_called ? 8u : 0u);
      const size_t row_off = row * A.plane_pitch;

      // the next row's lines (the row above or below, by the side), asked for before this row's barriers and consumed after them
      uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
      if (d < limit && touch_at <= A.touch_last) {
        const size_t next = up ? row + 1 : row - 1, at = next * A.plane_pitch + touch_at;
        t0 = *reinterpret_cast<const uint32_t*>(A.p0 + at);
        if constexpr (CALLED)
          if (!A.row_gap || A.row_gap[next] != 0) t3 = *reinterpret_cast<const uint32_t*>(A.pc + at);
        if constexpr (PLANES >= 2)
          if (!A.row_hi || A.row_hi[next] != 0) {
            t1 = *reinterpret_cast<const uint32_t*>(A.p1 + at);
            if constexpr (PLANES >= 3) t2 = *reinterpret_cast<const uint32_t*>(A.p2 + at);
          }
      }

      const uint32_t K_row = K;
      bool highs_clear = false;  // the row's last relabel left the high halves of the members' words 0
      for (uint32_t p = 0; p < 4 && K < n_act; ++p) {
        if (!((steps >> p) & 1u)) continue;
        uint32_t* bitmap = cur ? bitmap1 : bitmap0;
        uint32_t* other = cur ? bitmap0 : bitmap1;
        if (p == 0) {
          // the row's first step: read the member's state, park it, mark
#pragma unroll 4
          for (uint32_t r = tid; r < n; r += T) {
            const uint32_t l = label[r] & 0xFFFFu;
            if (l == kEhhNoClass) continue;
            const uint32_t bits = ehh_state<PLANES, CALLED>(A, row_off, A.cols[r], read_called, read_p1, read_p2);
            label[r] = l | (bits << 16);
            hap_mark(bitmap, 2u * l + (bits & 1u));
          }
        } else {
          for (uint32_t r = tid; r < n; r += T) {
            const uint32_t lw = label[r];
            if ((lw & 0xFFFFu) == kEhhNoClass) continue;
            hap_mark(bitmap, 2u * (lw & 0xFFFFu) + ((lw >> (16 + p)) & 1u));
          }
        }
        __syncthreads();
        // scan: every thread sums a contiguous chunk of the bitmap's words, the chunk sums are scanned over the wave and the waves
        const uint32_t W = (2u * K + 31u) >> 5;
        const uint32_t chunk = (W + T - 1) >> log2_T;
        const uint32_t lo = min(tid * chunk, W), hi = min(lo + chunk, W);
        uint32_t local = 0;
        for (uint32_t i = lo; i < hi; ++i) local += __popc(bitmap[i]);
        uint32_t incl = local;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t t = __shfl_up(incl, o);
          incl += t & (uint32_t)((int32_t)((uint32_t)o - 1u - lane) >> 31);  // lanes >= o, without a lane mask per distance
        }
        if (lane == 63u) s_wsum[wave] = incl;
        for (uint32_t i = tid; i < dirty_words; i += T) other[i] = 0;  // what the previous step marked
        __syncthreads();
        uint32_t base = 0, K_new = 0;
        for (uint32_t v = 0; v < waves; ++v) {
          const uint32_t t = s_wsum[v];
          K_new += t;
          if (v < wave) base += t;
        }
        dirty_words = W;
        cur ^= 1u;
        if (K_new == K) continue;  // nothing split: the dense rank of the keys is the identity
        uint32_t run = base + incl - local;
        for (uint32_t i = lo; i < hi; ++i) {
          prefix[i] = run;
          run += __popc(bitmap[i]);
        }
        __syncthreads();
        const uint32_t keep = (steps >> (p + 1)) ? 0xFFFF0000u : 0u;  // after the row's last step the parked state is of no more use
        for (uint32_t r = tid; r < n; r += T) {
          const uint32_t lw = label[r];
          if ((lw & 0xFFFFu) == kEhhNoClass) continue;
          const uint32_t key = 2u * (lw & 0xFFFFu) + ((lw >> (16 + p)) & 1u);
          label[r] = (lw & keep) | (prefix[key >> 5] + __popc(bitmap[key >> 5] & ((1u << (key & 31u)) - 1u)));
        }
        highs_clear = keep == 0u;
        // the boundary between the cores: the rank of core 1's first old key (2 B < 2 K lies inside the scanned words)
        B = B < K ? prefix[(2u * B) >> 5] + __popc(bitmap[(2u * B) >> 5] & ((1u << ((2u * B) & 31u)) - 1u)) : K_new;
        K = K_new;
      }
      asm volatile("" ::"v"(t0), "v"(t1), "v"(t2), "v"(t3));

      if (K != K_row) {
        // recount: class sizes into the high halves of label[0 .. K), then sum c (c - 1) / 2 per core.  The high halves are 0 already
        // where the row's last step relabelled (a word without a class keeps 0 from the pass below that read its count)
        if (!highs_clear)
          for (uint32_t r = tid; r < n; r += T) label[r] &= 0xFFFFu;
        __syncthreads();
        // A few large classes hold most of a wave's 64 members (one class, while K is small), and 64 adds to one word run one after the
        // other: the classes of the first four distinct lanes are counted over the wave and added once each, the lanes left add singly.
        for (uint32_t r0 = tid - lane; r0 < n; r0 += T) {  // the same trips for every lane of a wave
          const uint32_t r = r0 + lane;
          const uint32_t l = r < n ? label[r] & 0xFFFFu : kEhhNoClass;
          unsigned long long todo = __ballot(l != kEhhNoClass);
          for (int round = 0; round < 4 && todo; ++round) {
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t ll = __shfl(l, (int)leader);
            const unsigned long long same = __ballot(l == ll) & todo;
            if (lane == leader) atomicAdd(&label[ll], (uint32_t)__popcll(same) << 16);
            todo &= ~same;
          }
          if ((todo >> lane) & 1ull) atomicAdd(&label[l], 0x10000u);
        }
        __syncthreads();
        uint32_t q0 = 0, q1 = 0;  // a core's pairs are below 2^30
        for (uint32_t i = tid; i < K; i += T) {
          const uint32_t lw = label[i];  // the thread's own word
          label[i] = lw & 0xFFFFu;
          const uint32_t c = lw >> 16;
          const uint32_t pairs = c * (c - 1u) / 2u;  // c >= 1
          if (i < B) q0 += pairs; else q1 += pairs;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          q0 += __shfl_xor(q0, o);
          q1 += __shfl_xor(q1, o);
        }
        if (lane == 0) {
          s_red[2 * wave] = q0;
          s_red[2 * wave + 1] = q1;
        }
        __syncthreads();
        q0 = q1 = 0;
        for (uint32_t v = 0; v < waves; ++v) {
          q0 += s_red[2 * v];
          q1 += s_red[2 * v + 1];
        }
        P0 = q0;
        P1 = q1;
      }

      // rules 2 and 3, core 0 then core 1
      if (alive & 1u) {
        if (P0 * A.den < P_init0 * A.num) {
          alive &= ~1u;
        } else {
          area0 += (prev0 + P0) * gap;
          psteps0 += P0;
          steps0 = (uint32_t)d;
          if (curve && tid == 0) curve[d - 1] = (uint32_t)P0;
          if (P0 == 0) alive &= ~1u;
        }
      }
      if (alive & 2u) {
        if (P1 * A.den < P_init1 * A.num) {
          alive &= ~2u;
        } else {
          area1 += (prev1 + P1) * gap;
          psteps1 += P1;
          steps1 = (uint32_t)d;
          if (curve && tid == 0) curve[(size_t)A.max_extent + (d - 1)] = (uint32_t)P1;
          if (P1 == 0) alive &= ~2u;
        }
      }
      prev0 = P0;
      prev1 = P1;
      alive = __builtin_amdgcn_readfirstlane(alive);
    }
    flags |= alive * kEhhEdge0;  // still alive at max_extent or at the end of the range

    if (tid == 0) {
      EhhSide* o = A.out + item;
      o->area2[0] = area0; o->area2[1] = area1;
      o->pair_steps[0] = psteps0; o->pair_steps[1] = psteps1;
      o->steps[0] = steps0; o->steps[1] = steps1;
      o->core[0] = n0; o->core[1] = n1;
      o->flags = flags;
      o->reserved = 0;
    }
    if (curve) {  // the entries past each core's last counted step
      for (size_t i = (size_t)steps0 + tid; i < A.max_extent; i += T) curve[i] = 0;
      for (size_t i = (size_t)steps1 + tid; i < A.max_extent; i += T) curve[(size_t)A.max_extent + i] = 0;
    }
  }
}

}  // namespace fmh
