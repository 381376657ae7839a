// plane_rows.hpp — what the kernels of the device statistics and their host frame (stat_call.hpp) both see: how a kernel is handed the packed
// image of a matrix - the head of HapArgs, EhhArgs, FstatArgs, QcArgs, AssocArgs, ScoreArgs, RohArgs, IbdStateArgs, ClumpArgs and ClumpPairArgs (SfsArgs holds the same fields with its masks between
// them); the host fills it in one place, set_plane_rows - and the LDS of a compute unit.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace fmh {

struct PlaneRows {
  const uint8_t *p0, *p1, *p2, *pc;  // planes (p1 / p2 / pc may be null)
  const uint8_t *row_gap, *row_hi;   // one byte per row or null (null = read the plane of every row)
  size_t plane_pitch;
};

constexpr size_t kLdsPerCu = (size_t)160 << 10;  // MI355X

}  // namespace fmh
