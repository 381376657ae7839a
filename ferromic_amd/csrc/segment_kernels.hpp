// segment_kernels.hpp — the device side the segment statistics share (runs of homozygosity: roh_kernels.hpp, IBD segments:
// ibd_kernels.hpp): a thread's 16 bytes of the four planes of a kept row and the `called` fields derived from them, the per-kept-row plane
// flags, the record a (row block, owner) leaves, the rule that joins the blocks' records, and the append of a segment through the device
// counter.  One rule in one place: a third segment statistic includes this header and writes its own walk; grm_kernels.hpp takes the fetch
// and the plane flags for its code image.  (A kernel declared here is
// emitted into every unit that includes the header: what score_kernels.hpp shares with these, the plane load, is in plane_rows.hpp.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_rows.hpp"
#include "segment_host.hpp"  // run_qualifies: the same definition on the host and on the device

namespace fmh {

using fmh_host::run_qualifies;

// ---- a thread's 16 bytes of a kept row ------------------------------------------------------------------------------------------------------
constexpr uint32_t kSegGroupSamples = 256;  // matrix samples of a fetching workgroup: 64 bytes of a plane row
constexpr uint32_t kSegNone = 0xFFFFFFFFu;  // no list position (rank), no run (a record's head_last / tail_first)

struct PlaneStage {
  uint4 w0, wc, w1, w2;
};
// the four words of a stage: `b` of plane 0, and bit 2 s of called(q) = sample s of word q is called: both bits of the called plane set,
// no bit of the upper planes
struct PlaneFields {
  uint32_t b[4], pc[4], hi[4];
  __device__ __forceinline__ explicit PlaneFields(const PlaneStage& g)
      : b{g.w0.x, g.w0.y, g.w0.z, g.w0.w}, pc{g.wc.x, g.wc.y, g.wc.z, g.wc.w}, hi{g.w1.x | g.w2.x, g.w1.y | g.w2.y, g.w1.z | g.w2.z, g.w1.w | g.w2.w} {}
  __device__ __forceinline__ uint32_t called(int q) const { return pc[q] & (pc[q] >> 1) & ~(hi[q] | (hi[q] >> 1)) & kEvenBits; }
};
// `ok`: the row and the vector exist (else every field reads as not called); `fl`: the row's plane flags (plane_flags_kernel)
__device__ __forceinline__ PlaneStage plane_fetch(const PlaneRows& R, size_t off, bool ok, uint32_t fl) {
  PlaneStage g;
  g.w0 = plane_load(R.p0, off, ok, 0u);
  g.wc = plane_load(R.pc, off, ok && (fl & 1u), ok ? ~0u : 0u);
  g.w1 = plane_load(R.p1, off, ok && (fl & 2u) && R.p1, 0u);
  g.w2 = plane_load(R.p2, off, ok && (fl & 2u) && R.p2, 0u);
  return g;
}

// per kept row: which planes a fetch has to read of it, bit 0 the called plane, bit 1 the upper planes (the matrix's per-row tables are
// skip hints; without a table the plane is read)
static __global__ __launch_bounds__(256) void plane_flags_kernel(const PlaneRows R, size_t row_begin, const uint32_t* __restrict__ rows, uint32_t K,
                                                                 uint8_t* __restrict__ flags) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const size_t row = row_begin + rows[k];
  const uint32_t gap = R.pc ? (R.row_gap ? (R.row_gap[row] != 0) : 1u) : 0u;
  const uint32_t high = (R.p1 || R.p2) ? (R.row_hi ? (R.row_hi[row] != 0) : 1u) : 0u;
  flags[k] = (uint8_t)(gap | (high << 1));
}

// ---- the record of a (row block, owner): u32 fields [head_last, head_c[NC], tail_first, tail_c[NC], runs, sites], u64 [length, longest] -----
// head = the partial run that touches the block's first row, tail = the one that touches its last row (tail_first == b0: the whole block
// is one run, no head then), c = the NC counts a run carries (ROH: het, missing; IBD: missing); runs .. longest tally the block's interior
// runs.  Field f of block rb and owner `slot` is at [(rb * n32 + f) * stride + slot].
template <uint32_t NC> struct SegRec {
  static constexpr uint32_t head_last = 0, head_c = 1, tail_first = 1 + NC, tail_c = 2 + NC, runs = 2 + 2 * NC, sites = 3 + 2 * NC, n32 = 4 + 2 * NC;
};
constexpr uint32_t kSegRec64 = 2;

// The block-join rule.  One thread walks an owner's blocks in order and joins the tail of block r to the head of block r + 1 iff both exist
// and there is no break at the boundary: break(k) is bit k + brk_offset of `brk`.  judge(first, last, counts) gets every run that touches a
// block boundary, whole; interior(rb, r32) adds block rb's interior tallies, in block order (a block that is one run has none).
// `rec32` is the owner's field 0 of block 0.
template <uint32_t NC, class Judge, class Interior>
__device__ __forceinline__ void seg_stitch(const uint32_t* rec32, size_t stride, uint32_t n_blocks, uint32_t item_rows, uint32_t K,
                                           const unsigned long long* brk, uint32_t brk_offset, Judge judge, Interior interior) {
  using Rec = SegRec<NC>;
  bool carry = false;  // a run that touches the last row of the block before
  uint32_t c_first = 0, c[NC] = {}, head[NC];
  for (uint32_t rb = 0; rb < n_blocks; ++rb) {
    const uint32_t b0 = rb * item_rows;
    const uint32_t* r32 = rec32 + (size_t)rb * Rec::n32 * stride;
    const uint32_t head_last = r32[Rec::head_last * stride], tail_first = r32[Rec::tail_first * stride];
    const uint64_t at = (uint64_t)b0 + brk_offset;
    const bool joined = carry && !((brk[at >> 6] >> (at & 63)) & 1ull);
    if (tail_first == b0) {  // the whole block is one run
      if (!joined) {
        if (carry) judge(c_first, b0 - 1, c);
        carry = true; c_first = b0;
        for (uint32_t q = 0; q < NC; ++q) c[q] = 0;
      }
      for (uint32_t q = 0; q < NC; ++q) c[q] += r32[(Rec::tail_c + q) * stride];
      continue;  // no interior run
    }
    if (head_last != kSegNone) {
      for (uint32_t q = 0; q < NC; ++q) head[q] = r32[(Rec::head_c + q) * stride];
      if (joined) {
        for (uint32_t q = 0; q < NC; ++q) c[q] += head[q];
        judge(c_first, head_last, c);
      } else {
        if (carry) judge(c_first, b0 - 1, c);
        judge(b0, head_last, head);
      }
    } else if (carry) judge(c_first, b0 - 1, c);
    carry = false;
    interior(rb, r32);
    if (tail_first != kSegNone) {
      carry = true; c_first = tail_first;
      for (uint32_t q = 0; q < NC; ++q) c[q] = r32[(Rec::tail_c + q) * stride];
    }
  }
  if (carry) judge(c_first, K - 1, c);
}

// ---- a qualifying run, appended: the counter stays exact past the capacity; make() builds the segment only where it is stored --------------
// A holds `counter` (null = segments are neither counted nor stored), `segments` (device, `capacity` elements, or null) and `capacity`.
template <class Args, class Make>
__device__ __forceinline__ void seg_append(const Args& A, Make make) {
  if (!A.counter) return;
  const unsigned long long at = atomicAdd(A.counter, 1ull);
  if (A.segments && at < A.capacity) A.segments[at] = make();
}

}  // namespace fmh
