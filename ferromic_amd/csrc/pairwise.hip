// pairwise.hip — fmh_pairwise_differences: the sample-pair Gram contraction on the matrix cores (kernels in
// pairwise_kernels.hpp).  Its own translation unit so that it builds in parallel with the sweep routes.  It also defines gram_plan and
// gram_launch of gram_launch.hpp - how a Gram is sized and launched, shared with fmh_kinship_counts - beside the only instantiations of
// the Gram kernels, and fmh_timing_read_gram.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "abi_internal.hpp"
#include "pairwise_kernels.hpp"
#include "gram_launch.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace fmhi {

thread_local double g_gram_stage_ms[4] = {0.0, 0.0, 0.0, 0.0};

// max_product: the largest |a * b| of two operand values (pairwise: ploidy^2; kinship: 1).  An item's accumulators must stay exact - int32 on
// the int8 route, integers up to 2^24 in f32 on FP4 - so an item takes at most (2^24 | 2^31 - 1) / max_product sites: with max_product = 1
// that is 2^24 sites per item on FP4 and 2^31 - 1 on int8.
hipError_t gram_plan(Workspace* w, int device, const GramFormat& f, size_t n_pad, uint32_t n_samples, size_t k_bytes, size_t max_product,
                     GramPlan* out) {
  using namespace fmh;
  hipError_t e = hipSuccess;
  GramPlan p{};
  p.n_pad = n_pad;
  p.k_bytes = k_bytes;
  p.n_samples = n_samples;
  p.nt = n_pad / kPdBig;
  p.tiles = p.nt * (p.nt + 1) / 2;
  const bool fp4 = f.fp4, phased = f.phased;
  // persistent grid: as many workgroups per CU as are resident, dealt round-robin to the 8 XCDs; K is cut into 8 * j slices, j per XCD, sized so
  // that every XCD has several rounds of (slice, tile pair) items (balance) but a slice still spans many stages
  static thread_local int gram_occ[64][2];
  if (gram_occ[device][fp4] == 0) {
    int occ = 0;
    hipError_t oe = hipFuncSetAttribute(fp4 ? (const void*)pd_gram256_kernel<4, 4, true> : (const void*)pd_gram256_kernel<4, 4, false>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kPdBigStageBytes);
    if (oe == hipSuccess) oe = fp4 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pd_gram256_kernel<4, 4, true>, 1024, 2 * kPdBigStageBytes)
                                   : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pd_gram256_kernel<4, 4, false>, 1024, 2 * kPdBigStageBytes);
    if (oe != hipSuccess || occ < 1) occ = 1;
    gram_occ[device][fp4] = occ;
  }
  // FMH_PD_OCC is read on every call (the hardware's answer above is what is kept), so fmh_set_option takes effect in a running process;
  // like the other FMH_PD_* options it comes from the call's snapshot (gram_format), not from a fresh read per plan
  const int env_occ = (int)f.occ_cap;
  const int occ_now = env_occ > 0 && gram_occ[device][fp4] > env_occ ? env_occ : gram_occ[device][fp4];
  static thread_local bool phased_ready[64][2];
  if (phased && !phased_ready[device][fp4]) {
    e = hipFuncSetAttribute(fp4 ? (const void*)pd_gram256p_kernel<true> : (const void*)pd_gram256p_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kPdPhaseLdsBytes);
    if (e != hipSuccess) return e;
    phased_ready[device][fp4] = true;
  }
  // persistent: every workgroup resident (the phased kernel's two K tiles of LDS leave one workgroup per CU)
  p.grid = phased ? (unsigned)std::max(8, w->cus / 8 * 8) : (unsigned)std::max(8, w->cus * occ_now / 8 * 8);
  const size_t slots = p.grid / 8;
  const size_t env_chunk = (size_t)f.kchunk;
  size_t j = env_chunk ? std::max<size_t>(1, (k_bytes + 8 * env_chunk - 1) / (8 * env_chunk)) : std::max<size_t>(1, (slots * 8 + p.tiles - 1) / p.tiles);
  const size_t cap_sites = (fp4 ? ((size_t)1 << 24) : (((size_t)1 << 31) - 1)) / max_product;
  const size_t k_cap = std::max<size_t>(cap_sites / f.spb / kPdStageK, 1) * kPdStageK;
  size_t k_chunk = round_up((k_bytes + 8 * j - 1) / (8 * j), kPdStageK);
  const size_t k_floor = std::min<size_t>(k_bytes, 4096);  // at least 32 stages per item unless the slab is shorter
  if (k_chunk < k_floor) k_chunk = k_floor;
  if (k_chunk > k_cap) k_chunk = k_cap;
  j = ((k_bytes + k_chunk - 1) / k_chunk + 7) / 8;
  p.j = j;
  p.k_chunk = k_chunk;
  // the phased kernel writes every item's partial tile as a plain slab and a second kernel sums the slabs (no atomics) when the slabs fit the budget
  p.use_slabs = false;
  if (phased && f.slabs != 0) {
    const size_t slab_bytes = p.tiles * 8 * j * (size_t)kPdBig * kPdBig * sizeof(int);
    if (slab_bytes <= (size_t)f.slab_bytes) {
      if (w->pd_slab_bytes < slab_bytes) {
        // (hipFree waits for the device: a Gram enqueued earlier that still writes the old block has finished)
        if (w->pd_slabs) (void)hipFree(w->pd_slabs);
        w->pd_slabs = nullptr;
        w->pd_slab_bytes = 0;
        if ((e = hipMalloc((void**)&w->pd_slabs, slab_bytes)) != hipSuccess) return e;
        w->pd_slab_bytes = slab_bytes;
      }
      p.use_slabs = true;  // (read from the workspace at launch: a later plan of the same call may have grown the block)
    }
  }
  *out = p;
  return hipSuccess;
}

hipError_t gram_launch(Workspace* w, const GramFormat& f, const GramPlan& p, const uint8_t* planes, int plane_begin, int plane_count, int negate,
                       unsigned long long* dst, unsigned long long* totals, hipStream_t st) {
  using namespace fmh;
  int* slabs = p.use_slabs ? w->pd_slabs : nullptr;
  if (f.phased) {
    if (f.fp4)
      hipLaunchKernelGGL((pd_gram256p_kernel<true>), dim3(p.grid), dim3(kPdPhaseThreads), kPdPhaseLdsBytes, st, planes, p.n_pad, p.k_bytes, plane_begin, plane_count,
                         p.k_chunk, (uint32_t)p.j, p.n_samples, negate, dst, totals, slabs);
    else
      hipLaunchKernelGGL((pd_gram256p_kernel<false>), dim3(p.grid), dim3(kPdPhaseThreads), kPdPhaseLdsBytes, st, planes, p.n_pad, p.k_bytes, plane_begin, plane_count,
                         p.k_chunk, (uint32_t)p.j, p.n_samples, negate, dst, totals, slabs);
    if (slabs && hipGetLastError() == hipSuccess) {
      const size_t threads = p.tiles * 16384;
      hipLaunchKernelGGL(pd_slab_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, slabs, (uint32_t)p.nt, (uint32_t)p.j, p.k_chunk, p.k_bytes,
                         p.n_samples, negate, dst, totals);
    }
    return hipGetLastError();
  }
  if (f.fp4)
    hipLaunchKernelGGL((pd_gram256_kernel<4, 4, true>), dim3(p.grid), dim3(1024), 2 * kPdBigStageBytes, st, planes, p.n_pad, p.k_bytes, plane_begin, plane_count,
                       p.k_chunk, (uint32_t)p.j, p.n_samples, negate, dst, totals);
  else
    hipLaunchKernelGGL((pd_gram256_kernel<4, 4, false>), dim3(p.grid), dim3(1024), 2 * kPdBigStageBytes, st, planes, p.n_pad, p.k_bytes, plane_begin, plane_count,
                       p.k_chunk, (uint32_t)p.j, p.n_samples, negate, dst, totals);
  return hipGetLastError();
}

}  // namespace fmhi

extern "C" int fmh_timing_read_gram(double* h_stage_ms) {
  if (!h_stage_ms) return fail(FMH_ERR_INVALID, "h_stage_ms is NULL");
  for (int i = 0; i < 4; ++i) h_stage_ms[i] = g_gram_stage_ms[i];
  return FMH_OK;
}

extern "C" int fmh_pairwise_differences(const fmh_matrix* m, size_t n_samples, unsigned long long* d_diff,
                                        unsigned long long* d_both, void* stream) {
  if (!m || !d_diff || !d_both) return fail(FMH_ERR_INVALID, "NULL argument");
  FMH_TRY(check_samples(nullptr, n_samples, m->samples));
  if (m->ploidy > 127) return fail(FMH_ERR_UNSUPPORTED, "pairwise differences support ploidy <= 127 (int8 operands), got %zu", m->ploidy);
  FMH_TRY(use_device(m->device));
  if (n_samples < 2 || m->variants == 0) return FMH_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n_alleles = (int)m->max_allele + 1;
  const bool missing = m->has_missing;
  // biallelic and nothing missing: one plane (allele 1) and an all-ones row after the last sample (pairwise_kernels.hpp)
  const bool env_two_planes = options().pd_two_planes.load() != 0;  // measurements / tests: the general route
  const bool single = !missing && n_alleles == 2 && !env_two_planes;
  const int n_planes = single ? 1 : (missing ? n_alleles + 2 : n_alleles);  // + genotype length, + valid flag only when calls can be missing
  const size_t n_pad = round_up(n_samples + (single ? 1 : 0), kPdBig);
  // counts 0..4 are exact in FP4 (e2m1): twice the MFMA rate of int8 at half the plane bytes (pairwise_kernels.hpp); format, layout, row slabs,
  // the planes workspace and every Gram launch below come from gram_launch.hpp, which fmh_kinship_counts shares
  const GramFormat gf = gram_format(m->ploidy <= 4);
  const bool fp4 = gf.fp4;
  const int layout = gf.layout;
  const size_t spb = gf.spb, ksites = gf.ksites;
  const size_t slab = gram_row_slab(gf, (size_t)n_planes * n_pad, m->variants);
  // a matrix with a packed image feeds the planes kernel its bit rows (1/8 of the bytes); FMH_LAYOUT=bytes keeps the u8 route
  // (a three-plane image, alleles 4..7, is unpacked slab by slab into scratch bytes and takes the u8 planes kernel)
  const bool packed_only = m->p0 && !(m->data && layout_bytes_forced());
  const bool from_packed = packed_only && !m->p2;
  const bool via_unpack = packed_only && m->p2;
  Workspace* w = nullptr;
  FMH_TRY(workspace(m->device, &w));
  std::lock_guard<std::mutex> busy(w->in_use);
  uint8_t* planes = nullptr;
  FMH_TRY(gram_planes(w, (size_t)n_planes * n_pad * slab / spb, &planes));
  hipError_t e = hipSuccess;
  DeviceScratch scratch(m->device, st);
  unsigned long long *d_gram = nullptr, *d_totals = nullptr;
  if (single) {
    const size_t gram_bytes = n_samples * n_samples * sizeof(unsigned long long), totals_bytes = n_samples * sizeof(unsigned long long);
    FMH_TRY(scratch.get(&d_gram, n_samples * n_samples));
    FMH_TRY(scratch.get(&d_totals, n_samples));
    HIP_TRY(hipMemsetAsync(d_gram, 0, gram_bytes, st));
    HIP_TRY(hipMemsetAsync(d_totals, 0, totals_bytes, st));
  }
  uint8_t* unpacked = nullptr;
  if (via_unpack) {
    HIP_TRY(hipMalloc((void**)&unpacked, std::min(slab, m->variants) * m->pitch));
  }
  GramStageTimer timer(st);
  for (size_t row0 = 0; row0 < m->variants && e == hipSuccess; row0 += slab) {
    const size_t rows = std::min(slab, m->variants - row0);
    if ((e = timer.mark(0)) != hipSuccess) break;
    const size_t s_pad = round_up(rows, ksites);  // sites
    const size_t k_bytes = s_pad / spb;           // K bytes per sample in this slab
    if (from_packed) {
      // bit rows are tiny in LDS: 256 samples per workgroup (64-byte row pieces for diploid samples), fewer when the three staged
      // planes of a K block would pass the CU's 160 KiB (int8 route from ploidy 14: 3 x 128 x 449 B).  Halving keeps sbp a power of
      // two, so n_pad stays a multiple of it; the kernel stages dword pieces where sbp x ploidy is a multiple of 32 bits and bytes elsewhere
      uint32_t sbp = 256;
      auto packed_bitb = [&](uint32_t s) { return ((size_t)s * m->ploidy + 7) / 8 + 1; };
      while (3 * ksites * packed_bitb(sbp) > kPdPlanesLdsMax && sbp > 4) sbp /= 2;
      const size_t bitb = packed_bitb(sbp);
      const size_t smem_p = 3 * ksites * bitb;
      const dim3 grid_p((unsigned)(s_pad / ksites), (unsigned)(n_pad / sbp));
      const uint8_t* q0 = m->p0 + row0 * m->plane_pitch;
      const uint8_t* q1 = m->p1 ? m->p1 + row0 * m->plane_pitch : nullptr;
      const uint8_t* qc = m->pc ? m->pc + row0 * m->plane_pitch : nullptr;
      const void* fn = fp4 ? (const void*)pd_planes_packed_kernel<true> : (const void*)pd_planes_packed_kernel<false>;
      if (smem_p > 64 * 1024 && (e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_p)) != hipSuccess) break;
      if (fp4)
        hipLaunchKernelGGL(pd_planes_packed_kernel<true>, grid_p, dim3(256), smem_p, st, q0, q1, qc, m->plane_pitch, rows, (uint32_t)n_samples,
                           (uint32_t)m->ploidy, n_alleles, n_planes, single ? 1 : 0, single ? 1 : 0, sbp, planes, n_pad, s_pad, layout);
      else
        hipLaunchKernelGGL(pd_planes_packed_kernel<false>, grid_p, dim3(256), smem_p, st, q0, q1, qc, m->plane_pitch, rows, (uint32_t)n_samples,
                           (uint32_t)m->ploidy, n_alleles, n_planes, single ? 1 : 0, single ? 1 : 0, sbp, planes, n_pad, s_pad, layout);
    } else {
      if (!m->data && !via_unpack) { e = hipErrorInvalidValue; break; }
      MatrixView mv{};
      mv.pitch = m->pitch;
      mv.columns = m->columns;
      mv.nvec = m->nvec;
      if (via_unpack) {
        if ((e = unpack_rows(m, row0, rows, unpacked, m->pitch, st)) != hipSuccess) break;
        mv.data = unpacked;
        mv.bits = m->pc ? m->pc + row0 * m->plane_pitch : nullptr;  // a called plane row has the bit order of a called bit-row
        mv.bits_pitch = m->plane_pitch;
      } else {
        mv.data = m->data + row0 * m->pitch;
        mv.bits = m->bits ? m->bits + row0 * m->bits_pitch : nullptr;
        mv.bits_pitch = m->bits_pitch;
      }
      // samples per planes workgroup: the tile's raw bytes (one K block of sites x sb x ploidy) stay within 32 KiB of LDS, so
      // four workgroups share a CU and one's loads overlap another's packing (measured, 1 M x 2 500 FP4: 64 KiB tiles 1.94 ms,
      // 32 KiB 1.76 ms, 16 KiB 1.97 ms)
      const uint32_t env_sb = (uint32_t)gf.sb;  // measurements
      uint32_t sb = env_sb ? env_sb : kPdBlock;
      while ((size_t)sb * m->ploidy * ksites > 32 * 1024 && sb > 4) sb /= 2;
      const size_t planes_smem = ksites * ((size_t)sb * m->ploidy + ((size_t)sb * m->ploidy + 7) / 8 + 1);
      const void* planes_fn = fp4 ? (const void*)pd_planes_kernel<true> : (const void*)pd_planes_kernel<false>;
      if (planes_smem > 64 * 1024 && (e = hipFuncSetAttribute(planes_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)planes_smem)) != hipSuccess) break;
      const dim3 planes_grid((unsigned)(s_pad / ksites), (unsigned)(n_pad / sb));
      if (fp4)
        hipLaunchKernelGGL(pd_planes_kernel<true>, planes_grid, dim3(256), planes_smem, st, mv, rows, (uint32_t)n_samples, (uint32_t)m->ploidy, n_alleles,
                           n_planes, single ? 1 : 0, single ? 1 : 0, sb, planes, n_pad, s_pad, layout);
      else
        hipLaunchKernelGGL(pd_planes_kernel<false>, planes_grid, dim3(256), planes_smem, st, mv, rows, (uint32_t)n_samples, (uint32_t)m->ploidy, n_alleles,
                           n_planes, single ? 1 : 0, single ? 1 : 0, sb, planes, n_pad, s_pad, layout);
    }
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = timer.mark(1)) != hipSuccess) break;
    // an item's accumulators stay exact for operand products up to ploidy^2 (the cap of gram_plan)
    GramPlan plan;
    if ((e = gram_plan(w, m->device, gf, n_pad, (uint32_t)n_samples, k_bytes, m->ploidy * m->ploidy, &plan)) != hipSuccess) break;
    auto gram = [&](int plane_begin, int plane_count, int negate, unsigned long long* dst, unsigned long long* totals = nullptr) {
      return gram_launch(w, gf, plan, planes, plane_begin, plane_count, negate, dst, totals, st);
    };
    if (single) {
      if ((e = gram(0, 1, 0, d_gram, d_totals)) != hipSuccess) break;
      continue;
    }
    // diff = sum len_i len_j - sum_a cnt_i(a) cnt_j(a)
    if ((e = gram(0, n_alleles, 1, d_diff)) != hipSuccess) break;
    if (missing) {
      if ((e = gram(n_alleles, 1, 0, d_diff)) != hipSuccess) break;
      if ((e = gram(n_alleles + 1, 1, 0, d_both)) != hipSuccess) break;
    }
  }
  if (e == hipSuccess) e = timer.mark(3);
  if (e == hipSuccess && single) {
    const size_t total = n_samples * n_samples;
    hipLaunchKernelGGL(pd_single_plane_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_diff, d_both, d_gram, d_totals,
                       (uint32_t)n_samples, (unsigned long long)m->ploidy, (unsigned long long)m->variants);
    e = hipGetLastError();
  } else if (e == hipSuccess && !missing) {
    const size_t total = n_samples * n_samples;
    hipLaunchKernelGGL(pd_constant_terms_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_diff, d_both, (uint32_t)n_samples,
                       (unsigned long long)m->variants * m->ploidy * m->ploidy, (unsigned long long)m->variants);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = timer.mark(-1);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) timer.read();
  if (unpacked) { if (e != hipSuccess) (void)hipStreamSynchronize(st); (void)hipFree(unpacked); }
  if (e != hipSuccess) return fail(FMH_ERR_HIP, "pairwise differences failed: %s", hipGetErrorString(e));
  scratch.settled = true;
  return FMH_OK;
}

