// stat_call.hpp — the host frame the device statistics share (ld.hip, sfs.hip, hap.hip, ehh.hip, fstat.hip, kinship.hip, qc.hip, assoc.hip, logistic.hip, score.hip, roh.hip, ibd.hip, clump.hip, ldscore.hip, grm.hip, lmm.hip, admix.hip;
// pca.hip and pairwise.hip take the checks, the timer and the scratch): the refusals several entry points word alike, the plane pointers of a
// kernel's arguments, the rows-per-item rule, the size of a persistent grid, the event timer, and StatCall - device, workspace, stream, scratch
// and timer of one call.  One rule in one place, so the units cannot drift apart.  What only the segment statistics share (roh.hip, ibd.hip)
// is in segment_call.hpp, on top of this.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "abi_internal.hpp"
#include "plane_rows.hpp"

namespace fmhi {

// ---- refusals.  An entry point calls them where the header lists the refusal: the order in which refusals fire is part of the C-ABI -------
// a sample list (every entry in the matrix, strictly ascending), or without one the first n_samples samples
inline int check_samples(const uint32_t* h_samples_or_null, size_t n_samples, size_t matrix_samples) {
  if (!h_samples_or_null) {
    if (n_samples > matrix_samples) return fail(FMH_ERR_INVALID, "n_samples %zu exceeds the matrix's %zu samples", n_samples, matrix_samples);
    return FMH_OK;
  }
  for (size_t i = 0; i < n_samples; ++i) {
    if (h_samples_or_null[i] >= matrix_samples)
      return fail(FMH_ERR_INVALID, "sample %u (entry %zu) is outside the matrix's %zu samples", h_samples_or_null[i], i, matrix_samples);
    if (i && h_samples_or_null[i] <= h_samples_or_null[i - 1]) return fail(FMH_ERR_INVALID, "the sample list is not strictly ascending at entry %zu", i);
  }
  return FMH_OK;
}

// rows [row_begin, row_begin + row_count) of a matrix of `variants` rows (a range whose end wraps is refused and printed as it was given)
inline int check_rows(size_t row_begin, size_t row_count, size_t variants) {
  if (row_begin > variants || row_count > variants - row_begin)
    return fail(FMH_ERR_INVALID, "rows [%zu, %zu) exceed the matrix's %zu variants", row_begin, row_begin + row_count, variants);
  return FMH_OK;
}

// a table of [begin, end) rows; `noun` names an entry in the message ("window", "block")
struct RowSpan { size_t begin, end; };
static_assert(sizeof(RowSpan) == 2 * sizeof(uint64_t), "a window or block of the C-ABI is two u64");
inline int check_row_spans(const RowSpan* spans, size_t n_spans, const char* noun, size_t variants) {
  for (size_t i = 0; i < n_spans; ++i)
    if (spans[i].begin > spans[i].end || spans[i].end > variants)
      return fail(FMH_ERR_INVALID, "rows [%zu, %zu) of %s %zu exceed the matrix's %zu variants", spans[i].begin, spans[i].end, noun, i, variants);
  return FMH_OK;
}

// the statistics read the bit planes only; `who_reads` opens the message ("kinship reads", "the f-statistics read")
inline int check_packed(const fmh_matrix* m, const char* who_reads) {
  if (!m->p0) return fail(FMH_ERR_UNSUPPORTED, "%s the bit-packed image: call fmh_matrix_pack first (the matrix holds u8 rows only)", who_reads);
  return FMH_OK;
}

// ---- kernel arguments: the packed image of `m` (fmh::PlaneRows, or a struct with fields of the same names) --------------------------------
// The two per-row tables are handed on only with the planes they speak for: a matrix whose planes were rewritten without a called plane, or
// without upper planes, may still hold a table from before.
template <class Args> inline void set_plane_rows(Args& a, const fmh_matrix* m) {
  a.p0 = m->p0; a.p1 = m->p1; a.p2 = m->p2; a.pc = m->pc;
  a.row_gap = m->pc ? m->row_gap : nullptr;
  a.row_hi = (m->p1 || m->p2) ? m->row_hi : nullptr;
  a.plane_pitch = m->plane_pitch;
}

// ---- rows per work item (FMH_*_ITEM_ROWS) and the items of a launch ------------------------------------------------------------------------
constexpr size_t kMaxItemRows = (size_t)1 << 30;  // an item's row count, and an LDS bin its rows are counted into, is 32 bits
inline size_t item_rows_of(const std::atomic<long long>& option, size_t default_rows) {
  const long long opt = option.load(std::memory_order_relaxed);
  return opt <= 0 ? default_rows : std::min<size_t>((size_t)opt, kMaxItemRows);
}
// an item index is 32 bits; `option_name` is what the caller can raise
inline int check_item_count(size_t n_items, const char* option_name) {
  if (n_items > ((size_t)1 << 31)) return fail(FMH_ERR_UNSUPPORTED, "more than 2^31 work items: raise %s", option_name);
  return FMH_OK;
}

// ---- the persistent grid ------------------------------------------------------------------------------------------------------------------
// Workgroups of the persistent grid: the workgroups a CU holds by LDS and by its 2 048 thread slots (at most eight) - and, when
// `kernel_or_null` is given, by the kernel's registers as the runtime reports them: a workgroup beyond what is resident starts only when
// another has walked all its items, and then walks its own alone.  FMH_GRID_PER_CU / FMH_GRID_BLOCKS override; never more than the items.
// `lds_bytes` is the DYNAMIC LDS of the launch; a kernel that declares its LDS statically passes it as `static_lds_bytes` (the occupancy query
// reads it from the kernel itself and must not be told it twice).
inline int persistent_grid(const void* kernel_or_null, unsigned threads, size_t lds_bytes, size_t n_items, int cus, size_t* grid_out, size_t static_lds_bytes = 0) {
  size_t per_cu = std::max<size_t>(1, std::min<size_t>({(size_t)8, fmh::kLdsPerCu / (lds_bytes + static_lds_bytes), (size_t)2048 / threads}));
  if (kernel_or_null) {
    int resident = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kernel_or_null, (int)threads, lds_bytes));
    if (resident > 0) per_cu = std::min(per_cu, (size_t)resident);
  }
  const long long opt_per_cu = options().grid_per_cu.load(std::memory_order_relaxed);
  if (opt_per_cu > 0) per_cu = (size_t)std::min<long long>(opt_per_cu, 32);
  size_t grid = (size_t)std::max(cus, 1) * per_cu;
  const long long opt_blocks = options().grid_blocks.load(std::memory_order_relaxed);
  if (opt_blocks > 0) grid = (size_t)std::min<long long>(opt_blocks, 1 << 20);
  *grid_out = std::min(grid, n_items);
  return FMH_OK;
}

// ---- HIP events around a call's kernels when fmh_timing_enable is on: N events bound N - 1 stages, read after the stream's synchronise ----
template <int N = 2> struct KernelTimer {
  hipEvent_t ev[N] = {};
  bool on = false;
  KernelTimer() = default;
  KernelTimer(const KernelTimer&) = delete;
  ~KernelTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  // one decision per start (fmh_timing_enable(n) times every n-th), event 0
  int start(hipStream_t st) {
    on = timing_enabled();
    if (!on) return FMH_OK;
    for (hipEvent_t& e : ev) if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ev[0], st));
    return FMH_OK;
  }
  int mark(int i, hipStream_t st) {
    if (on) HIP_TRY(hipEventRecord(ev[i], st));
    return FMH_OK;
  }
  int stop(hipStream_t st) { return mark(N - 1, st); }
  // stage i, between events i and i + 1; *ms is left alone while timing is off
  int elapsed(int i, double* ms) {
    if (!on) return FMH_OK;
    float f = 0.0f;
    HIP_TRY(hipEventElapsedTime(&f, ev[i], ev[i + 1]));
    *ms = f;
    return FMH_OK;
  }
  // first to last event, added to the library's kernel time (fmh_timing_read)
  int read() {
    if (!on) return FMH_OK;
    float f = 0.0f;
    HIP_TRY(hipEventElapsedTime(&f, ev[0], ev[N - 1]));
    timing_add(f);
    return FMH_OK;
  }
};

// ---- one call of a device statistic -----------------------------------------------------------------------------------------------------------
// begin() once the arguments are checked; upload() / zeroed() for the call's tables; start(), the kernels, [stop(), copies back], finish().
// Whatever fails on the way returns at once: the scratch is then not settled and its destructor waits for the stream before the blocks go back
// to the pool.
struct StatCall {
  Workspace* ws = nullptr;
  hipStream_t st = nullptr;
  DeviceScratch scratch;
  KernelTimer<> timer;
  bool stopped = false;

  int begin(int device, void* stream) {
    FMH_TRY(use_device(device));
    FMH_TRY(workspace(device, &ws));
    st = (hipStream_t)stream;
    scratch.device = device;
    scratch.stream = st;
    return FMH_OK;
  }
  // `count` elements of T on the device: a copy of the host array (of any element type of the same bytes), or zeros
  template <class T> int upload(const void* host, size_t count, T** dev) {
    FMH_TRY(scratch.get(dev, count));
    HIP_TRY(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return FMH_OK;
  }
  template <class T> int zeroed(size_t count, T** dev) {
    FMH_TRY(scratch.get(dev, count));
    HIP_TRY(hipMemsetAsync(*dev, 0, count * sizeof(T), st));
    return FMH_OK;
  }
  // the timed span: from start() to stop(); finish() stops a span that is still open.  A call may run several spans (ld.hip: one per chunk).
  int start() {
    scratch.settled = false;
    stopped = false;
    return timer.start(st);
  }
  int stop() {
    if (stopped) return FMH_OK;
    stopped = true;
    return timer.stop(st);
  }
  int finish() {
    FMH_TRY(stop());
    HIP_TRY(hipStreamSynchronize(st));
    scratch.settled = true;
    return timer.read();
  }
};

}  // namespace fmhi
