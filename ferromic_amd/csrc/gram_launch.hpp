// gram_launch.hpp — how the sample-pair Gram product of pairwise_kernels.hpp is sized and launched, once: operand format and planes layout,
// the planes workspace and its row slabs, occupancy, the persistent grid, K slices (`j`, `k_chunk`), the exactness cap, the slab scratch of the
// phased kernel.  fmh_pairwise_differences (pairwise.hip) and fmh_kinship_counts (kinship.hip) both go through it, so FMH_PD_INT8,
// FMH_PD_PHASED, FMH_PD_SLABS, FMH_PD_SLAB_BYTES, FMH_PD_PLANES_BYTES, FMH_PD_KCHUNK and FMH_PD_OCC mean the same thing to both.
// Include after abi_internal.hpp and pairwise_kernels.hpp.  gram_plan and gram_launch are defined in pairwise.hip, beside the only instantiations
// of the Gram kernels.  Every function wants the caller to hold the workspace's `in_use`.
#pragma once

#include <algorithm>
#include <vector>

namespace fmhi {

// The operand format and the Gram kernel of one call.
struct GramFormat {
  bool fp4;       // e2m1 operands on v_mfma_scale_f32_16x16x128_f8f6f4 (else int8 on v_mfma_i32_16x16x64_i8)
  bool phased;    // pd_gram256p_kernel and layout 1 of pd_plane_offset (else pd_gram256_kernel and layout 0)
  int layout;
  size_t spb;     // sites per byte of a plane row
  size_t ksites;  // sites per K block = per Gram stage
  // the options gram_plan sizes a launch by, as they stood when the call began: a call plans once per row slab and operand region, and
  // another thread may call fmh_set_option between two of its plans
  long long occ_cap, kchunk, slabs, slab_bytes;  // FMH_PD_OCC, FMH_PD_KCHUNK, FMH_PD_SLABS, FMH_PD_SLAB_BYTES
  long long sb;                                  // FMH_PD_SB: samples per workgroup of the u8 planes kernel (pairwise only)
};
// fp4_exact: every operand value of the call is exact in e2m1 (pairwise: counts up to ploidy <= 4; kinship: -1, 0, 1).  One snapshot of
// the FMH_PD_* options per call: every later decision of the call (gram_row_slab aside, which reads its one option once) comes from it.
inline GramFormat gram_format(bool fp4_exact) {
  GramFormat f;
  f.fp4 = fp4_exact && options().pd_int8.load() == 0;  // FMH_PD_INT8: measurements / tests, the int8 route
  // round 4: the phase-interleaved Gram kernel and its planes layout (K halves contiguous); FMH_PD_PHASED=0 keeps round 3's
  f.phased = options().pd_phased.load() != 0;
  f.layout = f.phased ? 1 : 0;
  f.spb = f.fp4 ? 2 : 1;
  f.ksites = fmh::kPdStageK * f.spb;
  f.occ_cap = options().pd_occ.load();
  f.kchunk = options().pd_kchunk.load();
  f.slabs = options().pd_slabs.load();
  f.slab_bytes = options().pd_slab_bytes.load();
  f.sb = options().pd_sb.load();
  return f;
}

// Sites are processed in slabs so that the sample-major planes stay within FMH_PD_PLANES_BYTES of HBM: the sites of one slab when a site
// takes `plane_rows` operand rows (planes x padded samples, summed over the call's operand regions)
inline size_t gram_row_slab(const GramFormat& f, size_t plane_rows, size_t sites) {
  const size_t budget = (size_t)options().pd_planes_bytes.load();
  const size_t slab = std::max<size_t>(budget / plane_rows, fmh::kPdStageK) / fmh::kPdStageK * f.ksites;
  return std::min(round_up(sites, f.ksites), slab);
}

// the workspace's planes buffer, grown to `bytes` (kept between calls; fmh_device_release_scratch frees it)
inline int gram_planes(Workspace* w, size_t bytes, uint8_t** out) {
  if (w->pd_planes_bytes < bytes) {
    if (w->pd_planes) (void)hipFree(w->pd_planes);
    w->pd_planes = nullptr;
    w->pd_planes_bytes = 0;
    HIP_TRY(hipMalloc((void**)&w->pd_planes, bytes));
    w->pd_planes_bytes = bytes;
  }
  *out = w->pd_planes;
  return FMH_OK;
}

// One Gram launch over an operand region of n_pad rows x k_bytes K bytes per plane.
struct GramPlan {
  size_t n_pad, k_bytes, nt, tiles;
  uint32_t n_samples;  // rows whose pairs are written (the all-ones row, if any, is row n_samples)
  unsigned grid;
  size_t j, k_chunk;
  bool use_slabs;  // the phased kernel writes per-item partial tiles into the workspace's pd_slabs (else: 64-bit atomics)
};

// max_product: the largest |a * b| of two operand values (pairwise: ploidy^2; kinship: 1).  An item's accumulators must stay exact - int32 on
// the int8 route, integers up to 2^24 in f32 on FP4 - so an item takes at most (2^24 | 2^31 - 1) / max_product sites: with max_product = 1
// that is 2^24 sites per item on FP4 and 2^31 - 1 on int8.
hipError_t gram_plan(Workspace* w, int device, const GramFormat& f, size_t n_pad, uint32_t n_samples, size_t k_bytes, size_t max_product, GramPlan* out);

// dst(i, j) += sign * sum over planes [plane_begin, plane_begin + plane_count) of `planes` of row i . row j, for i < j < n_samples (row-major
// [n_samples][n_samples]); totals[i] += row i . row n_samples when given
hipError_t gram_launch(Workspace* w, const GramFormat& f, const GramPlan& p, const uint8_t* planes, int plane_begin, int plane_count, int negate,
                       unsigned long long* dst, unsigned long long* totals, hipStream_t st);

// Measurement (fmh_timing_enable, read back with fmh_timing_read_gram): HIP events between the stages of one call - [0] the planes kernels,
// [1] the first Gram of a row slab with its slab reduce (pairwise: all its Grams), [2] the second Gram (kinship: W), [3] the finish kernel -
// summed over the row slabs.  Nothing is recorded unless timing is on.
extern thread_local double g_gram_stage_ms[4];
struct GramStageTimer {
  hipStream_t st;
  bool on;
  std::vector<hipEvent_t> ev;
  std::vector<int> stage;
  explicit GramStageTimer(hipStream_t s) : st(s), on(timing_enabled()) {}
  GramStageTimer(const GramStageTimer&) = delete;
  ~GramStageTimer() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  // what is enqueued from here to the next mark belongs to stage `s` (-1: nothing follows)
  hipError_t mark(int s) {
    if (!on) return hipSuccess;
    hipEvent_t e = nullptr;
    hipError_t err = hipEventCreate(&e);
    if (err != hipSuccess) return err;
    ev.push_back(e);
    stage.push_back(s);
    return hipEventRecord(e, st);
  }
  // after the stream has been synchronised
  void read() {
    if (!on) return;
    for (double& v : g_gram_stage_ms) v = 0.0;
    for (size_t i = 0; i + 1 < ev.size(); ++i) {
      float ms = 0.0f;
      if (stage[i] >= 0 && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) g_gram_stage_ms[stage[i]] += ms;
    }
  }
};

}  // namespace fmhi
