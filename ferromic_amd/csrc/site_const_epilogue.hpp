// site_const_epilogue.hpp — the per-site epilogue of the table form of the tiled sweep (sweep_kernel_tiled_prefix).
// Included by sweep_tiled_kernels.hpp only; every other route keeps finish_biallelic_site + site_epilogue (sweep_kernels.hpp), which stay
// the same-process reference of this file (FMH_PREFIX_COUNTS=0, FMH_TILED=0).
//
// The table form exists only for biallelic matrices without a called plane: n[p] == A.group_size[p] for every site of the launch, so every
// division of the dense and sparse formulas except fst = num / dxy divides by a launch constant.
//   * the constants - (double)n, 1/n, n/(n-1), n*n, 1/(n*n), (double)(n(n-1)), theta's 1/H(n-1), (double)(n1 n2) and the refined reciprocals
//     of the denominators - are computed once per workgroup into LDS (const_epilogue_init, the shape of wc_rcp_init) with the very IEEE
//     operations site_epilogue performs per site;
//   * a division by one of them is div_shared: the last three operations of hipcc's own sequence on the same operands, the same bits;
//   * the prefix counts exist for columns <= 65 535 (u16 entries), so c0^2 + c1^2 <= n^2, a1 r2 + r1 a2 <= n1 n2 and n(n-1) are below 2^32:
//     32-bit products and one v_cvt_f64_u32 give the values the u64 arithmetic of site_epilogue gives (kConstEpilogueMaxColumns; the launcher
//     refuses wider matrices);
//   * the formula pair is a template argument (kFormulaRuntime = read it from the arguments): the launcher resolves it, outside the tile loop;
//   * fst = num / dxy, the one division by a per-site value, is evaluated only when the track is requested.
// Every track and every LaneTotals accumulator receives the operands of site_epilogue in its operation order.
#pragma once

#include "sweep_kernels.hpp"

namespace fmh {

constexpr uint32_t kConstEpilogueMaxColumns = 65535;  // n^2 <= 65 535^2 = 4 294 836 225 < 2^32
static_assert((unsigned long long)kConstEpilogueMaxColumns * kConstEpilogueMaxColumns <= 0xFFFFFFFFull, "32-bit sums of squares and pair products");
constexpr int kFormulaRuntime = -1;

// per group (kCe* + p * kCeGroup), then the pair (2 * kCeGroup + ...)
enum ConstEpilogueSlot : int {
  kCeN = 0,       // (double)n
  kCeInvN,        // 1.0 / n
  kCeScale,       // n / (n - 1.0)
  kCeNn,          // n * n
  kCeInvNn,       // 1.0 / (n * n)
  kCeNnm1,        // (double)(n (n - 1))
  kCeTheta,       // diversity: 1.0 / H(n - 1), 0.0 when the harmonic number is not positive
  kCeRcpN,        // refined_rcp of kCeN, kCeNn, kCeNnm1
  kCeRcpNn,
  kCeRcpNnm1,
  kCeGroup
};
constexpr int kCePairN12 = 2 * kCeGroup, kCePairRcp = 2 * kCeGroup + 1, kCeDoubles = 2 * kCeGroup + 2;

__device__ __forceinline__ double* const_epilogue_table() {
  __shared__ double table[kCeDoubles];
  return table;
}

// Every thread of the block, before the tile loop; ends in a __syncthreads().  Wave p fills group p and wave 2 the pair: all lanes of a wave
// write the same value to the same word, every index into the kernel arguments is a compile-time constant (wc_rcp_init).  The reciprocals of
// n == 0 and n == 1 are infinities or NaNs that no site consumes (the n >= 2 / n != 0 tests of the epilogue are scalar conditions).
template <int P, int MODE>
__device__ __forceinline__ const double* const_epilogue_init(const SweepArgs& A) {
  static_assert(P <= 2, "one or two groups");
  double* table = const_epilogue_table();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (wave == p) {
      const uint32_t nu = A.group_size[p];
      const double n = (double)nu;
      const double nn = n * n;
      const double nnm1 = (double)(nu * (nu - 1u));
      double* g = table + p * kCeGroup;
      g[kCeN] = n;
      g[kCeInvN] = 1.0 / n;
      g[kCeScale] = n / (n - 1.0);
      g[kCeNn] = nn;
      g[kCeInvNn] = 1.0 / nn;
      g[kCeNnm1] = nnm1;
      double theta = 0.0;
      if constexpr ((MODE & kModeDiversity) != 0) {
        if (nu >= 2) { const double denom = A.harmonic[nu - 1]; theta = denom > 0.0 ? 1.0 / denom : 0.0; }
      }
      g[kCeTheta] = theta;
      g[kCeRcpN] = refined_rcp(n);
      g[kCeRcpNn] = refined_rcp(nn);
      g[kCeRcpNnm1] = refined_rcp(nnm1);
    }
  }
  if constexpr (P >= 2) {
    if (wave == 2) {
      const double n12 = (double)(A.group_size[0] * A.group_size[1]);
      table[kCePairN12] = n12;
      table[kCePairRcp] = refined_rcp(n12);
    }
  }
  __syncthreads();
  return table;
}

// finish_biallelic_site + site_epilogue<P, MODE, false, false> of one site whose called counts are the launch's group sizes.
// F / HF: the formula of the population totals and of the Hudson part (kFormulaRuntime: A.formula / A.hudson_formula_p1).
template <int P, int MODE, int F, int HF>
__device__ __forceinline__ void site_const_epilogue(const SweepArgs& A, const double* K, size_t out_idx, bool row_ok, const uint32_t (&alt)[P],
                                                    LaneTotals<P, MODE>& T) {
  static_assert(P <= 2 && (MODE & kModeWc) == 0, "one or two groups, not W&C");
  const int formula = F != kFormulaRuntime ? F : A.formula;
  const int hf = HF != kFormulaRuntime ? HF : (A.hudson_formula_p1 ? A.hudson_formula_p1 - 1 : A.formula);
  const bool dense = hf != kFormulaSparse;

  uint32_t n[P], c0[P], distinct[P];
  double ssq[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    n[p] = A.group_size[p];
    c0[p] = n[p] - alt[p];
    ssq[p] = (double)(c0[p] * c0[p] + alt[p] * alt[p]);
    distinct[p] = (c0[p] != 0 ? 1u : 0u) + (alt[p] != 0 ? 1u : 0u);
  }
  auto pi_by = [&](int f, int p) {
    const double* g = K + p * kCeGroup;
    if (f == kFormulaSparse) {  // pi_sparse
      const double sum_p2 = ssq[p] * g[kCeInvN] * g[kCeInvN];
      return g[kCeScale] * (1.0 - sum_p2);
    }
    if (f == kFormulaDense) {  // pi_dense_nomissing
      if (alt[p] == 0 || alt[p] == n[p]) return 0.0;
      return g[kCeScale] * (1.0 - ssq[p] * g[kCeInvNn]);
    }
    return g[kCeScale] * (1.0 - div_shared(ssq[p], g[kCeNn], g[kCeRcpNn]));  // pi_dense
  };

  double pi[P];
  bool pi_ok[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    pi_ok[p] = n[p] >= 2;
    double v = 0.0, v_pop = 0.0;
    if (pi_ok[p]) {
      v_pop = pi_by(formula, p);
      v = hf == formula ? v_pop : pi_by(hf, p);
    }
    pi[p] = v;
    if (row_ok) {
      if (pi_ok[p]) T.pop_pi[p] += v_pop; else T.pop_unc[p] += 1;
      if (distinct[p] >= 2) T.pop_seg[p] += 1;
      if (p < A.n_groups) {
        if (A.alt) site_store(A.alt + ((size_t)p * A.row_count + out_idx), alt[p]);
        if (A.called) site_store(A.called + ((size_t)p * A.row_count + out_idx), n[p]);
      }
    }
  }

  if constexpr ((MODE & kModeDiversity) != 0) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      double pv, tv;
      if (n[p] < 2) { pv = f64_nan(); tv = f64_nan(); }
      else {
        tv = distinct[p] > 1 ? K[p * kCeGroup + kCeTheta] : 0.0;
        pv = pi_by(kFormulaSparse, p);
      }
      if (row_ok && p < A.n_groups) {
        const size_t o = (size_t)p * A.row_count + out_idx;
        if (A.site_pi) site_store(A.site_pi + o, pv);
        if (A.site_theta) site_store(A.site_theta + o, tv);
        if (A.site_distinct) site_store(A.site_distinct + o, distinct[p]);
      }
    }
  }

  if constexpr ((MODE & kModeHudson) != 0 && P >= 2) {
    const double* g1 = K;
    const double* g2 = K + kCeGroup;
    const uint32_t n1 = n[0], n2 = n[1];
    const bool dxy_ok = (n1 != 0) && (n2 != 0);
    const double a1 = (double)alt[0], a2 = (double)alt[1], r1 = (double)c0[0], r2 = (double)c0[1];
    // the frequency dot product of dxy_from_counts (finish_biallelic_site), ascending allele order
    double hud_dot = 0.0;
    if (dxy_ok) {
      const double inv1 = g1[kCeInvN], inv2 = g2[kCeInvN];
      if (c0[0] != 0 && c0[1] != 0) hud_dot += (r1 * inv1) * (r2 * inv2);
      if (alt[0] != 0 && alt[1] != 0) hud_dot += (a1 * inv1) * (a2 * inv2);
    }
    double dxy = 0.0;
    if (dxy_ok) {
      if (dense) {  // dxy_dense_biallelic
        const double alt1_f = div_shared(a1, g1[kCeN], g1[kCeRcpN]);
        const double alt2_f = div_shared(a2, g2[kCeN], g2[kCeRcpN]);
        const double ref1 = 1.0 - alt1_f;
        const double ref2 = 1.0 - alt2_f;
        double dot = ref1 * ref2 + alt1_f * alt2_f;
        if (dot < 0.0) dot = 0.0;
        dxy = 1.0 - dot;
        if (dxy < 0.0) dxy = 0.0; else if (dxy > 1.0) dxy = 1.0;
      } else dxy = clamp01(1.0 - hud_dot);
    }
    double fst = f64_nan(), numc = f64_nan(), denc = f64_nan();
    bool comp_ok = false;
    if (dxy_ok && pi_ok[0] && pi_ok[1]) {
      if (dxy > kFstEps) {
        const double num = dxy - 0.5 * (pi[0] + pi[1]);
        if (A.fst) fst = num / dxy;  // the one division by a per-site value: only when its track is requested
        numc = num; denc = dxy; comp_ok = true;
      } else {
        const double pi_avg = 0.5 * (pi[0] + pi[1]);
        if (fabs(pi_avg) <= kFstEps) { numc = 0.0; denc = 0.0; comp_ok = true; }
      }
    }
    if (row_ok) {
      if (A.fst) site_store(A.fst + (out_idx), fst);
      if (A.dxy) site_store(A.dxy + (out_idx), dxy_ok ? dxy : f64_nan());
      if (A.pi1) site_store(A.pi1 + (out_idx), pi_ok[0] ? pi[0] : f64_nan());
      if (A.pi2) site_store(A.pi2 + (out_idx), pi_ok[1] ? pi[1] : f64_nan());
      if (A.num) site_store(A.num + (out_idx), numc);
      if (A.den) site_store(A.den + (out_idx), denc);
      if (comp_ok) { T.hud[5] += numc; T.hud[6] += denc; T.hud_u[1] += 1; }
      if (dxy_ok) T.hud[7] += clamp01(1.0 - hud_dot); else T.hud_u[2] += 1;
      // aggregate_hudson_components_from_summaries: n1 n2 != 0 and n (n - 1) > 0 follow from the scalar tests on n
      if (!dxy_ok) {
        T.hud_u[0] += 1;
      } else {
        double d = div_shared((double)(alt[0] * c0[1] + c0[0] * alt[1]), K[kCePairN12], K[kCePairRcp]);
        if (d < 0.0) d = 0.0; else if (d > 1.0) d = 1.0;
        T.hud[4] += d;
        if (n1 >= 2 && n2 >= 2) {
          const double p1 = div_shared(2.0 * a1 * r1, g1[kCeNnm1], g1[kCeRcpNnm1]);
          const double p2 = div_shared(2.0 * a2 * r2, g2[kCeNnm1], g2[kCeRcpNnm1]);
          T.hud[2] += p1;
          T.hud[3] += p2;
          if (d > kFstEps) { T.hud[0] += d - 0.5 * (p1 + p2); T.hud[1] += d; }
        }
      }
    }
  }
}

}  // namespace fmh
