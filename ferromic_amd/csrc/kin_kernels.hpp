// kin_kernels.hpp — gfx950 kernels of fmh_kinship_counts: bit planes -> genotype-class operand planes for the Gram kernels of
// pairwise_kernels.hpp, and the kernel that turns their sums into the four tables.  Include after pairwise_kernels.hpp (pd_plane_offset,
// pd_fp4_code, kPdStageK).  Definition and operand algebra: include/ferromic_hip.h (fmh_kinship_counts), DESIGN.md section 3.16.
#pragma once

namespace fmh {

// What kin_planes_kernel reads and writes.  Diploid samples: sample s owns columns 2 s and 2 s + 1, so its two bits of a plane row sit in ONE
// byte (bit 2 s & 7 of byte s >> 2).
struct KinPlanesArgs {
  const uint8_t *p0, *p1, *p2, *pc;  // bit planes of the matrix; p1, p2, pc may be null
  size_t plane_pitch;
  const unsigned long long* rows;    // kept rows of this slab (matrix row numbers), or null: row_first + i
  size_t row_first;
  size_t row_count;                  // kept rows in this slab; K positions from here to s_pad are zero
  const uint32_t* samples;           // the selected samples, or null: sample i is matrix sample i
  uint32_t n;                        // selected samples
  // region A (n_pad_a rows): H_i at row i, with `general` V_i at row n + i, then the all-ones row, then zero rows.
  // region W (n_pad_w rows, `w_offset` bytes after A): W_i = R_i - A_i at row i, then zero rows.
  int general;
  size_t n_pad_a, n_pad_w, w_offset;
  size_t s_pad;                      // K positions (sites) per row, a multiple of the K block
  int layout;
  uint8_t* planes;
};

// Workgroup = one K block (256 sites as FP4, 128 as int8) x 256 samples.  The 2-bit genotype fields of p0, (p1 | p2) and pc are staged in LDS as
// [site][64 bytes] - four samples per byte, sample s of the block at bits 2 (s & 3) of byte s >> 2.  With the identity sample list that is a
// dword copy of the plane rows (64-byte row pieces); a sample list gathers each field from its own byte.  A thread then turns one LDS byte
// column (four samples) x one 16-byte chunk of K into the samples' H, V and W chunks.  The planes may carry junk under uncalled entries: every
// class is ANDed with "both entries called and no upper-plane bit".
constexpr uint32_t kKinSb = 256;  // samples per workgroup
constexpr uint32_t kKinRowBytes = kKinSb / 4;

template <bool FP4>
__global__ __launch_bounds__(256) void kin_planes_kernel(const KinPlanesArgs a) {
  extern __shared__ __align__(16) unsigned char kin_smem[];
  constexpr uint32_t KS = FP4 ? 2 * kPdStageK : kPdStageK;  // sites per K block
  constexpr uint32_t PER = KS / 8;                          // sites per 16-byte chunk of an operand row
  uint8_t* l0 = kin_smem;                                   // [KS][64] each
  uint8_t* lh = l0 + (size_t)KS * kKinRowBytes;
  uint8_t* lc = lh + (size_t)KS * kKinRowBytes;
  const size_t kb = blockIdx.x, site0 = kb * KS;
  const uint32_t samp0 = blockIdx.y * kKinSb;
  auto row_of = [&](size_t i) { return a.rows ? (size_t)a.rows[i] : a.row_first + i; };
  if (!a.samples) {
    const size_t byte0 = (size_t)samp0 / 4;  // a multiple of 64
    for (uint32_t w = threadIdx.x; w < KS * (kKinRowBytes / 4); w += 256) {
      const uint32_t r = w / (kKinRowBytes / 4), c = (w % (kKinRowBytes / 4)) * 4;
      const bool ok = site0 + r < a.row_count && byte0 + c + 4 <= a.plane_pitch;
      const size_t off = ok ? row_of(site0 + r) * a.plane_pitch + byte0 + c : 0;
      const uint32_t v0 = ok ? *reinterpret_cast<const uint32_t*>(a.p0 + off) : 0u;
      uint32_t vh = ok && a.p1 ? *reinterpret_cast<const uint32_t*>(a.p1 + off) : 0u;
      if (ok && a.p2) vh |= *reinterpret_cast<const uint32_t*>(a.p2 + off);
      const uint32_t vc = ok ? (a.pc ? *reinterpret_cast<const uint32_t*>(a.pc + off) : 0xFFFFFFFFu) : 0u;
      *reinterpret_cast<uint32_t*>(l0 + (size_t)r * kKinRowBytes + c) = v0;
      *reinterpret_cast<uint32_t*>(lh + (size_t)r * kKinRowBytes + c) = vh;
      *reinterpret_cast<uint32_t*>(lc + (size_t)r * kKinRowBytes + c) = vc;
    }
  } else {
    // a thread owns one LDS byte column (four listed samples) and walks the rows: where the samples' fields sit is looked up once
    const uint32_t c = threadIdx.x % kKinRowBytes;
    uint32_t byte_of[4] = {0, 0, 0, 0}, shift_of[4] = {0, 0, 0, 0}, listed = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t s = samp0 + c * 4 + k;
      if (s < a.n) {
        const uint32_t col = a.samples[s] * 2u;
        byte_of[k] = col >> 3;
        shift_of[k] = col & 7u;
        listed = k + 1;
      }
    }
    for (uint32_t r = threadIdx.x / kKinRowBytes; r < KS; r += 256 / kKinRowBytes) {
      uint32_t v0 = 0, vh = 0, vc = 0;
      if (site0 + r < a.row_count) {
        const size_t base = row_of(site0 + r) * a.plane_pitch;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          if (k < listed) {
            const size_t off = base + byte_of[k];
            const uint32_t sh = shift_of[k];
            v0 |= (((uint32_t)a.p0[off] >> sh) & 3u) << (2 * k);
            uint32_t h = a.p1 ? (uint32_t)a.p1[off] : 0u;
            if (a.p2) h |= a.p2[off];
            vh |= ((h >> sh) & 3u) << (2 * k);
            vc |= (a.pc ? ((uint32_t)a.pc[off] >> sh) & 3u : 3u) << (2 * k);
          }
        }
      }
      l0[(size_t)r * kKinRowBytes + c] = (uint8_t)v0;
      lh[(size_t)r * kKinRowBytes + c] = (uint8_t)vh;
      lc[(size_t)r * kKinRowBytes + c] = (uint8_t)vc;
    }
  }
  __syncthreads();
  const size_t k_blocks = a.s_pad / KS;
  auto store = [&](size_t region, size_t n_pad, size_t row, uint32_t chunk, const uint32_t (&o)[4]) {
    *reinterpret_cast<uint4*>(a.planes + region + pd_plane_offset(a.layout, 0, k_blocks, kb, n_pad, row, chunk)) = make_uint4(o[0], o[1], o[2], o[3]);
  };
  // K position i of a 16-byte chunk: a nibble (FP4) or a byte (int8) of dword i / (PER / 4)
  constexpr int kPerDword = (int)PER / 4, kWidth = FP4 ? 4 : 8;
  for (uint32_t v = threadIdx.x; v < kKinRowBytes * 8; v += 256) {
    const uint32_t q = v % kKinRowBytes, chunk = v / kKinRowBytes;
    uint32_t h[4][4] = {}, hom[4][4] = {}, wv[4][4] = {};
#pragma unroll
    for (int i = 0; i < (int)PER; ++i) {
      const uint32_t r = chunk * PER + i;  // rows past the slab's end were staged as "not called"
      const uint32_t y0 = l0[(size_t)r * kKinRowBytes + q], yh = lh[(size_t)r * kKinRowBytes + q], yc = lc[(size_t)r * kKinRowBytes + q];
      // the four samples of the byte at once, one flag per sample at bits 0, 2, 4, 6 - plain integer arithmetic, no lane masks
      const uint32_t called = yc & (yc >> 1) & ~(yh | (yh >> 1)) & 0x55u;
      const uint32_t b0 = y0 & 0x55u, b1 = (y0 >> 1) & 0x55u;
      const uint32_t het = called & (b0 ^ b1), alt = called & b0 & b1, homf = called & ~(b0 ^ b1);
      const int d = i / kPerDword, sh = (i % kPerDword) * kWidth;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t fh = (het >> (2 * k)) & 1u, fv = (homf >> (2 * k)) & 1u, fa = (alt >> (2 * k)) & 1u;
        if constexpr (FP4) {
          // e2m1: 1 = code 0x2, -1 = code 0xA (the sign is bit 3)
          h[k][d] |= fh << (sh + 1);
          hom[k][d] |= fv << (sh + 1);
          wv[k][d] |= ((fv << 1) | (fa << 3)) << sh;
        } else {
          h[k][d] |= fh << sh;
          hom[k][d] |= fv << sh;
          wv[k][d] |= (fv | (fa * 0xFEu)) << sh;  // ref: 0x01, alt: 0xFF
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t s = samp0 + q * 4 + k;
      if (s < a.n) {
        store(0, a.n_pad_a, s, chunk, h[k]);
        if (a.general) store(0, a.n_pad_a, (size_t)a.n + s, chunk, hom[k]);
        store(a.w_offset, a.n_pad_w, s, chunk, wv[k]);
      } else if (s < a.n_pad_w) {  // zero rows from n to the W region's end
        const uint32_t zero[4] = {0, 0, 0, 0};
        store(a.w_offset, a.n_pad_w, s, chunk, zero);
      }
    }
  }
  auto put_one = [](uint32_t (&out)[4], int i) { out[i / kPerDword] |= (FP4 ? 0x2u : 0x1u) << ((i % kPerDword) * kWidth); };
  // the tail of region A, by the last sample block: the all-ones row (1 at every kept site of the slab), then zero rows
  if (blockIdx.y == gridDim.y - 1) {
    const size_t tail0 = a.general ? 2 * (size_t)a.n : (size_t)a.n;
    const size_t tail = a.n_pad_a - tail0;
    for (size_t v = threadIdx.x; v < tail * 8; v += 256) {
      const size_t row = tail0 + v / 8;
      const uint32_t chunk = (uint32_t)(v % 8);
      uint32_t o[4] = {0, 0, 0, 0};
      if (row == tail0) {
#pragma unroll
        for (int i = 0; i < (int)PER; ++i)
          if (site0 + chunk * PER + i < a.row_count) put_one(o, i);
      }
      store(0, a.n_pad_a, row, chunk, o);
    }
  }
}

// The four tables from the Gram sums, one thread per element (i, j), no atomics, ADDED into the caller's buffers.
//   general:  ga = [2 n][2 n], upper triangle of the self-Gram of [H; V]; ta[2 n] = the totals of H, then of V
//   complete: ga = [n][n], upper triangle of H . H; ta[n] = the totals of H; V = 1 - H over the `kept` rows
//   gw = [n][n], upper triangle of W . W (two's complement sums)
__global__ __launch_bounds__(256) void kin_finish_kernel(const unsigned long long* __restrict__ ga, const unsigned long long* __restrict__ ta,
                                                         const unsigned long long* __restrict__ gw, uint32_t n, int general, unsigned long long kept,
                                                         unsigned long long* __restrict__ both, unsigned long long* __restrict__ het_het,
                                                         unsigned long long* __restrict__ ibs0, unsigned long long* __restrict__ het_hom) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n * n) return;
  const uint32_t i = (uint32_t)(idx / n), j = (uint32_t)(idx % n);
  if (i == j) {
    both[idx] += general ? ta[i] + ta[n + i] : kept;
    het_het[idx] += ta[i];
    return;
  }
  const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
  unsigned long long hh, hv_ij, hv_ji, vv;
  if (general) {
    const size_t n2 = 2 * (size_t)n;
    hh = ga[(size_t)lo * n2 + hi];
    vv = ga[((size_t)n + lo) * n2 + n + hi];
    hv_ij = ga[(size_t)i * n2 + n + j];  // row i < column n + j for every i, j
    hv_ji = ga[(size_t)j * n2 + n + i];
  } else {
    hh = ga[(size_t)lo * n + hi];
    hv_ij = ta[i] - hh;
    hv_ji = ta[j] - hh;
    vv = kept - ta[i] - ta[j] + hh;
  }
  const unsigned long long ww = gw[(size_t)lo * n + hi];
  both[idx] += hh + hv_ij + hv_ji + vv;
  het_het[idx] += hh;
  ibs0[idx] += (vv - ww) >> 1;  // V . V - W . W = 2 (R_i . A_j + A_i . R_j) >= 0
  het_hom[idx] += hv_ij;
}

}  // namespace fmh
