// plane_rows.hpp — what the kernels of the device statistics and their host frame (stat_call.hpp) both see: how a kernel is handed the packed
// image of a matrix - the head of HapArgs, EhhArgs, FstatArgs, QcArgs, AssocArgs, ScoreArgs, RohArgs, IbdStateArgs, ClumpArgs, ClumpPairArgs, LdScoreArgs, GrmCodeArgs and LmmArgs (SfsArgs holds the same fields with its masks between
// them); the host fills it in one place, set_plane_rows - how a kernel reads 16 bytes of a plane row, and the LDS of a compute unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fmh {

struct PlaneRows {
  const uint8_t *p0, *p1, *p2, *pc;  // planes (p1 / p2 / pc may be null)
  const uint8_t *row_gap, *row_hi;   // one byte per row or null (null = read the plane of every row)
  size_t plane_pitch;
};

// 16 bytes of a plane row, or `fill` in every word where the plane is not read
__device__ __forceinline__ uint4 plane_load(const uint8_t* plane, size_t off, bool on, uint32_t fill) {
  uint4 v = make_uint4(fill, fill, fill, fill);
  if (on) v = *reinterpret_cast<const uint4*>(plane + off);
  return v;
}

// a diploid sample's 2-bit field of a plane word: sample s of the word at bits 2 s, 2 s + 1; the low bit of every field
constexpr uint32_t kEvenBits = 0x55555555u;

constexpr size_t kLdsPerCu = (size_t)160 << 10;  // MI355X

}  // namespace fmh
