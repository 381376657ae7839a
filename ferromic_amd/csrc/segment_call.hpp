// segment_call.hpp — what the host entry points of the segment statistics share on top of stat_call.hpp (roh.hip, ibd.hip): the refusals
// they word alike and SegmentFrame, what both put on the device besides their own scratch.  Each statistic keeps its own parameter check,
// scratch sizing, budget, grids and argument structs.
#pragma once

#include <string>
#include <vector>

#include "segment_host.hpp"
#include "segment_kernels.hpp"
#include "stat_call.hpp"

namespace fmhi {

// what the device and the host entry point refuse alike after the statistic's own parameter check: x = the positions of the rows, or null
inline int check_segment_request(const uint32_t* x, size_t x_count, bool any_table, const void* segments, const uint64_t* count) {
  for (size_t k = 1; x && k < x_count; ++k)
    if (x[k] < x[k - 1]) return fail(FMH_ERR_INVALID, "the positions descend at row entry %zu of the range", k);
  if (!any_table && !segments && !count) return fail(FMH_ERR_INVALID, "every output is NULL");
  if (segments && !count) return fail(FMH_ERR_INVALID, "a segment buffer is given but h_segment_count is NULL");
  return FMH_OK;
}

// Every refusal of a device scan, in the header's order, before any launch.  `noun` names the statistic ("runs of homozygosity", "IBD
// segments"); check_params() is the statistic's own check of *params and runs once params is known not to be NULL.
template <class CheckParams>
int check_segment_scan(const fmh_matrix* m, const void* params, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                       const uint32_t* h_positions_or_null, bool any_table, const void* segments, const uint64_t* count, const char* noun,
                       CheckParams check_params) {
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  FMH_TRY(check_params());
  FMH_TRY(check_segment_request(h_positions_or_null ? h_positions_or_null + row_begin : nullptr, row_count, any_table, segments, count));
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "%s take diploid genotypes (ploidy 2), got ploidy %zu", noun, m->ploidy);
  FMH_TRY(check_packed(m, (std::string(noun) + " read").c_str()));
  if (row_count >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "a range of %zu rows: fewer than 2^32 - 1 are taken (split the rows)", row_count);
  return FMH_OK;
}

// What both scans put on the device besides their own scratch: the kept rows and their positions, the break bitmap, per matrix sample of
// the groups of 256 through the last selected one its list position (kSegNone: not selected), the per-kept-row plane flags of a matrix
// with a called or an upper plane (null without either) and the counter the kernels append segments through (null when segments are
// neither counted nor stored).  The constructor is host work; upload() before call.start(), launch_flags() first among the kernels,
// finish() in place of call.finish(): it reads the count back behind the timed span and hands it to the caller.
struct SegmentFrame {
  fmh_host::KeptRows kept;
  uint32_t nvec;    // 16-byte vectors of a row through the last selected sample: 64 samples each; within the row, that sample exists
  uint32_t groups;  // ceil(nvec / 4)
  std::vector<uint32_t> rank;  // [groups * 256]
  uint32_t *d_rows = nullptr, *d_x = nullptr, *d_rank = nullptr;
  unsigned long long *d_brk = nullptr, *d_counter = nullptr;
  uint8_t* d_flags = nullptr;

  SegmentFrame(const uint8_t* h_keep_or_null, const uint32_t* h_positions_or_null, size_t row_begin, size_t row_count, const uint32_t* h_samples_or_null, size_t n)
      : kept(fmh_host::kept_rows(h_keep_or_null, h_positions_or_null, row_begin, row_count)) {
    const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
    nvec = last / 64 + 1;
    groups = (nvec + 3) / 4;
    rank.assign((size_t)groups * fmh::kSegGroupSamples, fmh::kSegNone);
    for (size_t i = 0; i < n; ++i) rank[h_samples_or_null ? h_samples_or_null[i] : i] = (uint32_t)i;
  }
  static bool has_flags(const fmh_matrix* m) { return m->pc || m->p1 || m->p2; }
  int upload(StatCall& call, const fmh_matrix* m, const std::vector<unsigned long long>& brk, bool segments) {
    FMH_TRY(call.upload(kept.rows.data(), kept.rows.size(), &d_rows));
    FMH_TRY(call.upload(kept.x.data(), kept.x.size(), &d_x));
    FMH_TRY(call.upload(brk.data(), brk.size(), &d_brk));
    FMH_TRY(call.upload(rank.data(), rank.size(), &d_rank));
    if (segments) FMH_TRY(call.zeroed(1, &d_counter));
    if (has_flags(m)) FMH_TRY(call.scratch.get(&d_flags, kept.rows.size()));
    return FMH_OK;
  }
  int launch_flags(StatCall& call, const fmh_matrix* m, size_t row_begin) {
    if (!d_flags) return FMH_OK;
    const size_t K = kept.rows.size();
    fmh::PlaneRows planes{};
    set_plane_rows(planes, m);
    hipLaunchKernelGGL(fmh::plane_flags_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, call.st, planes, row_begin, d_rows, (uint32_t)K, d_flags);
    HIP_TRY(hipGetLastError());
    return FMH_OK;
  }
  int finish(StatCall& call, uint64_t* h_segment_count) {
    FMH_TRY(call.stop());
    unsigned long long count = 0;
    if (d_counter) HIP_TRY(hipMemcpyAsync(&count, d_counter, sizeof count, hipMemcpyDeviceToHost, call.st));
    FMH_TRY(call.finish());
    if (h_segment_count) *h_segment_count = count;
    return FMH_OK;
  }
};

}  // namespace fmhi
