// hap_kernels.hpp — haplotype homozygosity windows (Garud's H) from the packed bit planes: the identical-haplotype classes of one group over
// row windows (hap.hip; definition in include/ferromic_hip.h, scheme and measurements in DESIGN.md section 3.13).
//
// One workgroup owns one window; a persistent grid walks the windows by block stride.  The partition of the n members lives in LDS and is
// refined one binary step per plane per row (planes p0 & pc, p1 & pc, p2 & pc, pc; the planes a matrix does not have, and those row_hi /
// row_gap say a row leaves empty, are skipped):
//   mark     key = 2 label + bit; bit `key` of a presence bitmap of 2 K bits is set (read first, LDS atomic OR only when it is not set yet:
//            bits are only ever set, and while K is small every member hits the same word)
//   scan     the popcounts of the bitmap's ceil(2 K / 32) words are prefix-summed over the workgroup: K_new and one prefix per word
//   relabel  only if K_new != K (keys are monotone in the label, so without a split the dense rank is the identity):
//            label = prefix[key >> 5] + popc(bitmap[key >> 5] & below(key))
// Two bitmaps alternate, the one a step leaves dirty is cleared during the scan of the next step: a step that splits nothing costs two
// barriers, one that splits costs three.  A window stops refining once K == n.
//
// Member rank r (ascending column) belongs to thread r % threads for the whole launch; its column comes from the table `cols` (built on
// the host).  A label is below n < 2^16, so a member's LDS word holds it in the low half.  The high half is free while a window is refined:
// the pass that marks a row's first step reads the member's bit of every plane ONCE and parks the four bits there, so the later steps of the
// row and every relabel read LDS only.  At the end of a window the high halves take the class sizes (LDS atomic add) and then, when the
// partition is asked for, the smallest member rank of each class (LDS atomic min).  Outputs leave with plain stores: nothing else writes a
// window's record.  Loops over members have no per-member registers, so one instantiation serves every workgroup size and group size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_rows.hpp"

namespace fmh {

// the record of include/ferromic_hip.h's fmh_hap_window
struct HapWindow {
  unsigned long long sum_sq;
  uint32_t distinct;
  uint32_t top[3];
};

struct HapArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  const uint32_t* cols;              // [n]: the column of member rank r, ascending
  uint32_t n;
  uint32_t touch_first, touch_last;  // byte offsets of the first and last plane dword of a row that holds a member
  const unsigned long long* windows; // [n_windows][2]: rows [begin, end)
  unsigned long long n_windows;
  HapWindow* out;                    // [n_windows]
  uint32_t* first;                   // [n_windows][n] or null
};

constexpr uint32_t kHapLdsHead = 128;       // dwords before the labels: 16 wave sums of the scan, 16 x 6 of the end-of-window reduction
// the largest group: head + n labels + 3 x ceil(n / 16) words (two bitmaps of 2 n bits, one prefix per bitmap word) within 160 KiB
constexpr uint32_t kHapMaxMembers = 34304;

__host__ __device__ constexpr uint32_t hap_pad4(uint32_t x) { return (x + 3u) & ~3u; }
__host__ __device__ constexpr uint32_t hap_bitmap_words(uint32_t n) { return hap_pad4((n + 15u) / 16u); }
__host__ __device__ constexpr size_t hap_lds_bytes(uint32_t n) { return ((size_t)kHapLdsHead + hap_pad4(n) + 3u * (size_t)hap_bitmap_words(n)) * 4u; }
static_assert(hap_lds_bytes(kHapMaxMembers) <= kLdsPerCu, "the largest group fits one CU's LDS");
static_assert(kHapMaxMembers < 0xFFFFu, "labels, class sizes and member ranks are 16-bit halves of an LDS word");

__device__ __forceinline__ void hap_top3_insert(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t v) {
  // a >= b >= c stays sorted; branch-free (the branchy form made the compiler index the three as an array in scratch)
  const uint32_t below_a = min(a, v);
  a = max(a, v);
  const uint32_t below_b = min(b, below_a);
  b = max(b, below_a);
  c = max(c, below_b);
}

// bit `key` of the presence bitmap: read first, the LDS atomic only when the bit is not set yet
__device__ __forceinline__ void hap_mark(uint32_t* bitmap, uint32_t key) {
  const uint32_t bit = 1u << (key & 31u);
  if (!(bitmap[key >> 5] & bit)) atomicOr(&bitmap[key >> 5], bit);
}

// Launched with 64, 256, 512 or 1 024 threads and hap_lds_bytes(n) of dynamic LDS.  PLANES = the allele planes of the matrix (1..3), CALLED =
// it has a called plane: compile-time, because every test of a null plane pointer inside the loops is a lane mask the compiler keeps in a
// pair of SGPRs, and the kernel ran out of them.
template <int PLANES, bool CALLED>
__global__ __launch_bounds__(1024) void hap_kernel(const HapArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hap_lds[];
  const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = T >> 6;
  const uint32_t log2_T = 31u - (uint32_t)__clz((int)T);  // T is a power of two
  const uint32_t n = A.n, nw = hap_bitmap_words(n);
  uint32_t* s_wsum = hap_lds;
  uint32_t* s_red = hap_lds + 16;
  uint32_t* label = hap_lds + kHapLdsHead;  // [n]: low half = the member's label, high half = see the head of this file
  uint32_t* bitmap0 = label + hap_pad4(n);
  uint32_t* bitmap1 = bitmap0 + nw;
  uint32_t* prefix = bitmap1 + nw;
  const uint32_t touch_at = A.touch_first + tid * 128u;  // next row's lines are fetched ahead, one dword per line, by the first threads

  for (unsigned long long w = blockIdx.x; w < A.n_windows; w += gridDim.x) {
    const size_t row_begin = (size_t)A.windows[2 * w], row_end = (size_t)A.windows[2 * w + 1];
    __syncthreads();  // the previous window's last reads of label[]
    for (uint32_t r = tid; r < n; r += T) label[r] = 0;
    for (uint32_t i = tid; i < 2 * nw; i += T) bitmap0[i] = 0;  // both bitmaps
    __syncthreads();
    uint32_t K = 1, cur = 0, dirty_words = 0;

    for (size_t row = row_begin; row < row_end && K < n; ++row) {
      const bool read_called = CALLED && (!A.row_gap || A.row_gap[row] != 0);
      const bool read_p1 = PLANES >= 2 && (!A.row_hi || A.row_hi[row] != 0), read_p2 = PLANES >= 3 && read_p1;
      const uint32_t steps = 1u | (read_p1 ? 2u : 0u) | (read_p2 ? 4u : 0u) | (read_called ? 8u : 0u);
      const size_t row_off = row * A.plane_pitch;

      // the next row's lines, asked for before this row's barriers and consumed after them
      uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
      if (row + 1 < row_end && touch_at <= A.touch_last) {
        const size_t next = row + 1, at = next * A.plane_pitch + touch_at;
        t0 = *reinterpret_cast<const uint32_t*>(A.p0 + at);
        if constexpr (CALLED)
          if (!A.row_gap || A.row_gap[next] != 0) t3 = *reinterpret_cast<const uint32_t*>(A.pc + at);
        if constexpr (PLANES >= 2)
          if (!A.row_hi || A.row_hi[next] != 0) {
            t1 = *reinterpret_cast<const uint32_t*>(A.p1 + at);
            if constexpr (PLANES >= 3) t2 = *reinterpret_cast<const uint32_t*>(A.p2 + at);
          }
      }

      for (uint32_t p = 0; p < 4 && K < n; ++p) {
        if (!((steps >> p) & 1u)) continue;
        uint32_t* bitmap = cur ? bitmap1 : bitmap0;
        uint32_t* other = cur ? bitmap0 : bitmap1;
        if (p == 0) {
          // the row's first step: read the member's state (bits 0..2 = allele bits under the called plane, bit 3 = called), park it, mark
#pragma unroll 4
          for (uint32_t r = tid; r < n; r += T) {
            const uint32_t c = A.cols[r];
            const size_t at = row_off + (size_t)(c >> 5) * 4;
            const uint32_t sh = c & 31u;
            uint32_t called = 1u;
            if (read_called) called = (*reinterpret_cast<const uint32_t*>(A.pc + at) >> sh) & 1u;
            uint32_t bits = (*reinterpret_cast<const uint32_t*>(A.p0 + at) >> sh) & 1u;
            if (read_p1) bits |= ((*reinterpret_cast<const uint32_t*>(A.p1 + at) >> sh) & 1u) << 1;
            if (read_p2) bits |= ((*reinterpret_cast<const uint32_t*>(A.p2 + at) >> sh) & 1u) << 2;
            bits = called ? (bits | 8u) : 0u;
            const uint32_t l = label[r] & 0xFFFFu;
            label[r] = l | (bits << 16);
            hap_mark(bitmap, 2u * l + (bits & 1u));
          }
        } else {
          for (uint32_t r = tid; r < n; r += T) {
            const uint32_t lw = label[r];
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
        for (uint32_t r = tid; r < n; r += T) {
          const uint32_t lw = label[r];
          const uint32_t key = 2u * (lw & 0xFFFFu) + ((lw >> (16 + p)) & 1u);
          label[r] = (lw & 0xFFFF0000u) | (prefix[key >> 5] + __popc(bitmap[key >> 5] & ((1u << (key & 31u)) - 1u)));
        }
        K = K_new;
      }
      asm volatile("" ::"v"(t0), "v"(t1), "v"(t2), "v"(t3));
    }

    // class sizes into the high halves of label[0 .. K)
    for (uint32_t r = tid; r < n; r += T) label[r] &= 0xFFFFu;
    __syncthreads();
    for (uint32_t r = tid; r < n; r += T) atomicAdd(&label[label[r] & 0xFFFFu], 0x10000u);
    __syncthreads();
    unsigned long long sum_sq = 0;
    uint32_t c1 = 0, c2 = 0, c3 = 0;
    for (uint32_t i = tid; i < K; i += T) {
      const uint32_t c = label[i] >> 16;
      sum_sq += (unsigned long long)c * c;
      hap_top3_insert(c1, c2, c3, c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum_sq += __shfl_xor(sum_sq, o);
      const uint32_t o1 = __shfl_xor(c1, o), o2 = __shfl_xor(c2, o), o3 = __shfl_xor(c3, o);
      hap_top3_insert(c1, c2, c3, o1);
      hap_top3_insert(c1, c2, c3, o2);
      hap_top3_insert(c1, c2, c3, o3);
    }
    if (lane == 0) {
      uint32_t* red = s_red + wave * 6;
      red[0] = (uint32_t)sum_sq;
      red[1] = (uint32_t)(sum_sq >> 32);
      red[2] = c1; red[3] = c2; red[4] = c3;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long total = 0;
      uint32_t a = 0, b = 0, c = 0;
      for (uint32_t v = 0; v < waves; ++v) {
        const uint32_t* red = s_red + v * 6;
        total += (unsigned long long)red[0] | ((unsigned long long)red[1] << 32);
        hap_top3_insert(a, b, c, red[2]);
        hap_top3_insert(a, b, c, red[3]);
        hap_top3_insert(a, b, c, red[4]);
      }
      HapWindow* o = A.out + w;
      o->sum_sq = total;
      o->distinct = K;
      o->top[0] = a; o->top[1] = b; o->top[2] = c;
    }
    if (A.first) {
      // the smallest member rank of each class into the high halves, then every member reads its class's
      for (uint32_t i = tid; i < K; i += T) label[i] |= 0xFFFF0000u;
      __syncthreads();
      for (uint32_t r = tid; r < n; r += T) {
        const uint32_t l = label[r] & 0xFFFFu;
        atomicMin(&label[l], (r << 16) | (label[l] & 0xFFFFu));  // the low half of a word does not change in this phase
      }
      __syncthreads();
      uint32_t* first = A.first + (size_t)w * n;
      for (uint32_t r = tid; r < n; r += T) first[r] = label[label[r] & 0xFFFFu] >> 16;
    }
  }
}

}  // namespace fmh
