// sweep_tiled_kernels.hpp — the sweep over the TILE-TRANSPOSED image of plane 0 (fmh_matrix::p0t): packed biallelic
// matrices with nothing missing, one or two groups, every mode but W&C; and its table form over the prefix counts (fmh_matrix::p0c, section
// 3.5d; sweep_kernel_tiled_prefix at the end of the file).  Included by sweep_tiled.hip only.
//
//   * the image: the 16 bytes of row r, vector v live at byte (((r >> 6) * pvec + v) * 64 + (r & 63)) * 16 - the 64 rows of an image tile share
//     the lines of one vector column, so a column window of `n` vectors is n contiguous KiB per tile and every byte of every fetched line
//     belongs to a row and a vector the sweep needs (row-major, a 20-vector window of a 40-vector row fetches three 128-byte lines for 2.5);
//   * tile -> wave -> lane as in tiles_pipelined: tiles are 64 rows relative to row_begin, lane L owns relative row 64 * tile + L and computes
//     its own address from its absolute row, so a tile that straddles two image tiles is two contiguous pieces per load instruction;
//   * one 16-byte-per-lane load per window vector, 1 KiB contiguous per wave instruction; the masks are wave-uniform: scalar loads from the
//     bit-mask image (mask_bits), AND with an SGPR source, v_bcnt accumulate - no cross-lane reduction, no select;
//   * a derived group (SweepArgs::derived_group) is not counted at all: the kernels are built for C counted groups of the P reported ones;
//   * the window is walked in batches of 2 x HB vectors held as two halves: while one half is counted the other is in flight, and the loads of
//     the next tile's first batch are issued under the last batch's counting and land under the epilogue (the shape of tiles_pipelined);
//   * finish_biallelic_site, site_epilogue, the stores and reduce_block_totals are the other routes': lane L's sites in tile order, so the
//     order of every f64 sum is the four-lane route's at the same grid.
#pragma once

#include "site_const_epilogue.hpp"
#include "sweep_kernels.hpp"

namespace fmh {

typedef const __attribute__((address_space(4))) uint32_t* tiled_cptr_t;  // constant address space: uniform loads are s_load

template <int P, int MODE, int C, int HB>
__global__ __launch_bounds__(kBlock) void sweep_kernel_tiled(const SweepArgs A) {
  static_assert(P <= 2 && C <= P && C >= P - 1 && (MODE & kModeWc) == 0, "one or two groups, at most one of them derived, not W&C");
  constexpr int B = 2 * HB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  LaneTotals<P, MODE> T;
  T.clear();
  const size_t ntiles = (A.row_count + kTileRows - 1) / kTileRows;
  const size_t tile_stride = (size_t)gridDim.x * kWavesPerBlock;
  size_t tile = (size_t)blockIdx.x * kWavesPerBlock + (size_t)wave;
  if (tile < ntiles) {
    const uint32_t W = A.mv.nvec, last = W - 1;      // the window: A.mv.data and A.mask_bits start at its first vector
    const uint32_t nb = (W + B - 1) / B;
    const size_t image_tile = A.mv.pitch * kTileRows;  // bytes of one image tile: 1 KiB per vector of the whole row
    // the counted group(s): both, the only one, or the one that is not derived
    const int cg = C == P ? 0 : 1 - A.derived_group;
    const uint32_t mstride = (uint32_t)(A.mask_pitch / 32);  // dwords between the bit masks of two groups
    const tiled_cptr_t mk = (tiled_cptr_t)(uintptr_t)A.mask_bits + (size_t)cg * mstride;
    // The rows of relative tile t: a uniform base (the image tile of the tile's first row, at the window's first vector) and this lane's 32-bit
    // offset from it - its slot in the image tile, one image tile further when the tile straddles two.  Rows past the end re-read the last one
    // (their results are discarded).
    const uint32_t image_tile32 = (uint32_t)image_tile;
    auto tile_base = [&](size_t t, const uint8_t*& sbase, uint32_t& loff) {
      const size_t row0 = A.row_begin + t * kTileRows;
      const size_t rel = t * kTileRows + (size_t)lane;
      const size_t row = A.row_begin + (rel < A.row_count ? rel : A.row_count - 1);
      sbase = A.mv.data + (row0 >> 6) * image_tile;
      loff = (uint32_t)((row >> 6) - (row0 >> 6)) * image_tile32 + (uint32_t)(row & 63) * 16u;
    };
    // Vectors past the window (the last batch of a window that is no multiple of the batch) re-read its last one against a zero mask; a half that
    // lies inside the window is counted without the clamps.  (c0 is made opaque: the compiler otherwise hoists
    // the clamped offsets, mask addresses and keep-words of every vector of the loop-invariant last batch out of the tile loop, 60 SGPRs and more
    // that it then spills into VGPR lanes.)
    auto load_half = [&](uint4 (&dst)[HB > 0 ? HB : 1], const uint8_t* sbase, uint32_t loff, uint32_t c0) {
      asm volatile("" : "+s"(c0));
#pragma unroll
      for (int u = 0; u < HB; ++u) {
        const uint32_t c = c0 + u;
        dst[u] = load_stream(sbase + (size_t)(loff + (c < last ? c : last) * 1024u));  // (two image tiles of at most 1.6 MB: 32 bits)
      }
    };
    // (The masks are the same for every tile: an opaque pointer that also passes the running count keeps the s_loads of each pair of vectors
    // behind the counting of the pair before it - eight to sixteen SGPRs of masks at a time, every load a scalar-cache hit - instead of a whole
    // half's, or a whole window's hoisted out of the tile loop, in SGPRs the epilogue's kernel arguments need.)
    auto count_half = [&](const uint4 (&x)[HB > 0 ? HB : 1], uint32_t c0, uint32_t (&cnt)[C > 0 ? C : 1]) {
      asm volatile("" : "+s"(c0));
      if (c0 + HB <= W) {
        tiled_cptr_t mh = mk + (size_t)c0 * 4;
#pragma unroll
        for (int u = 0; u < HB; ++u) {
          if (u % 2 == 0) asm volatile("" : "+s"(mh), "+v"(cnt[0]));
          const tiled_cptr_t m = mh + u * 4;
#pragma unroll
          for (int q = 0; q < C; ++q) {
            cnt[q] = bcnt_add(x[u].x & m[(size_t)q * mstride + 0], cnt[q]);
            cnt[q] = bcnt_add(x[u].y & m[(size_t)q * mstride + 1], cnt[q]);
            cnt[q] = bcnt_add(x[u].z & m[(size_t)q * mstride + 2], cnt[q]);
            cnt[q] = bcnt_add(x[u].w & m[(size_t)q * mstride + 3], cnt[q]);
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < HB; ++u) {
          const uint32_t c = c0 + u;
          const uint32_t keep = c < W ? 0xFFFFFFFFu : 0u;
          tiled_cptr_t m = mk + (size_t)(c < last ? c : last) * 4;
          asm volatile("" : "+s"(m), "+v"(cnt[0]));
#pragma unroll
          for (int q = 0; q < C; ++q) {
            cnt[q] = bcnt_add(x[u].x & (m[(size_t)q * mstride + 0] & keep), cnt[q]);
            cnt[q] = bcnt_add(x[u].y & (m[(size_t)q * mstride + 1] & keep), cnt[q]);
            cnt[q] = bcnt_add(x[u].z & (m[(size_t)q * mstride + 2] & keep), cnt[q]);
            cnt[q] = bcnt_add(x[u].w & (m[(size_t)q * mstride + 3] & keep), cnt[q]);
          }
        }
      }
    };
    uint4 a[HB > 0 ? HB : 1], b[HB > 0 ? HB : 1];
    const uint8_t* base;
    uint32_t loff;
    tile_base(tile, base, loff);
    if constexpr (C > 0) {
      load_half(a, base, loff, 0);
      load_half(b, base, loff, HB);
    }
    for (; tile < ntiles; tile += tile_stride) {
      const size_t nxt = tile + tile_stride < ntiles ? tile + tile_stride : tile;  // after the last tile: its own rows once more (L2 hits, unused)
      const uint8_t* nbase;
      uint32_t nloff;
      tile_base(nxt, nbase, nloff);
      uint32_t cnt[C > 0 ? C : 1];
#pragma unroll
      for (int q = 0; q < (C > 0 ? C : 1); ++q) cnt[q] = 0;
      const uint32_t row_alt = load_row_alt(A, tile * kTileRows, lane);  // issued before the tile's vectors, consumed after them
      if constexpr (C > 0) {
        for (uint32_t k = 0; k + 1 < nb; ++k) {
          count_half(a, k * B, cnt);
          load_half(a, base, loff, (k + 1) * B);
          count_half(b, k * B + HB, cnt);
          load_half(b, base, loff, (k + 1) * B + HB);
        }
        // the last batch of this tile; the first of the next one goes out under it and lands under the epilogue
        count_half(a, (nb - 1) * B, cnt);
        load_half(a, nbase, nloff, 0);
        count_half(b, (nb - 1) * B + HB, cnt);
        load_half(b, nbase, nloff, HB);
      }
      base = nbase;
      loff = nloff;
      uint32_t alt_mine[P];
      if constexpr (C == P) {
#pragma unroll
        for (int p = 0; p < P; ++p) alt_mine[p] = cnt[p];
      } else {
#pragma unroll
        for (int p = 0; p < P; ++p) alt_mine[p] = C > 0 && p == cg ? cnt[0] : 0u;
      }
      derive_group<P>(A.derived_group, row_alt, alt_mine);
      SiteTally<P> mine;
      WcSite<P> wc;
      double hud_dot = 0.0;
#pragma unroll
      for (int p = 0; p < P; ++p) { mine.n[p] = A.group_size[p]; mine.alt[p] = alt_mine[p]; mine.distinct[p] = 0; mine.ssq[p] = 0; }
      mine.n_all = A.mv.columns;
      finish_biallelic_site<P, MODE>(mine, hud_dot);
      const size_t my_rel = tile * kTileRows + (size_t)lane;
      site_epilogue<P, MODE, false, false>(A, my_rel, my_rel < A.row_count, mine, hud_dot, wc, T);
    }
  }
  reduce_block_totals<P, MODE>(A, T);
}

// The table form: every counted group is one column range, so its whole vectors are two entries of the prefix counts
// (A.prefix: for image tile T, boundary b and row slot s the u16 at ((T * (pvec + 1) + b) * 64 + s) - 128 contiguous bytes per wave
// instruction) and only the at most two vectors the range shares with other columns are read from the image and counted, under masks that
// arrive as kernel arguments.  A group with no whole vector loads no entry, one with no shared vector loads no vector (all wave-uniform).
// Tile -> wave -> lane, the clamp of the rows past the end, derive_group, the stores and reduce_block_totals are sweep_kernel_tiled's.  The
// epilogue is site_const_epilogue (site_const_epilogue.hpp): every called count of this form is a launch constant, so
// the divisions of finish_biallelic_site + site_epilogue by them share their reciprocals - the same integers reach the same f64 operations in
// the same order and give the same bits.  F / HF: the launch's formula pair, resolved by the launcher (kFormulaRuntime = read from the arguments
// inside the loop), so a built pair has no branch on the formula in its tile loop and registers for its own arms only.  The next tile's loads
// are issued before this tile's epilogue and land under it.
template <int P, int MODE, int C, int F, int HF>
__global__ __launch_bounds__(kBlock) void sweep_kernel_tiled_prefix(const SweepArgs A) {
  static_assert(P <= 2 && C <= P && C >= P - 1 && C >= 1 && (MODE & kModeWc) == 0, "one or two groups, at most one of them derived, not W&C");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  LaneTotals<P, MODE> T;
  T.clear();
  const double* K0 = const_epilogue_init<P, MODE>(A);  // the launch constants of the epilogue, in LDS (ends in a barrier)
  const size_t ntiles = (A.row_count + kTileRows - 1) / kTileRows;
  const size_t tile_stride = (size_t)gridDim.x * kWavesPerBlock;
  size_t tile = (size_t)blockIdx.x * kWavesPerBlock + (size_t)wave;
  if (tile < ntiles) {
    const uint32_t pvec = (uint32_t)(A.mv.pitch / 16);
    const int cg = C == P ? 0 : 1 - A.derived_group;
    struct TileIn {
      uint32_t row_alt, hi[C], lo[C];
      uint4 e[C][2];
    };
    // this lane's row of relative tile t (rows past the end re-read the last one: their results are discarded), its image tile and its slot there
    auto load_tile = [&](size_t t, TileIn& in) {
      const size_t rel = t * kTileRows + (size_t)lane;
      const size_t row = A.row_begin + (rel < A.row_count ? rel : A.row_count - 1);
      const size_t it = row >> 6, slot = row & 63;
      in.row_alt = A.derived_group >= 0 ? A.row_alt[row] : 0u;
      const uint16_t* pc = A.prefix + it * ((size_t)pvec + 1) * 64 + slot;
      const uint8_t* px = A.mv.data + (it * pvec * 64 + slot) * 16;
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const PrefixGroup& g = A.prefix_group[q];
        in.hi[q] = g.b_hi ? (uint32_t)pc[(size_t)g.b_hi * 64] : 0u;
        in.lo[q] = g.b_lo ? (uint32_t)pc[(size_t)g.b_lo * 64] : 0u;
#pragma unroll
        for (int k = 0; k < 2; ++k) in.e[q][k] = (uint32_t)k < g.n_edges ? load_stream(px + (size_t)g.edge_vec[k] * 1024) : make_uint4(0, 0, 0, 0);
      }
    };
    TileIn in;
    load_tile(tile, in);
    for (; tile < ntiles; tile += tile_stride) {
      uint32_t cnt[C];
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const PrefixGroup& g = A.prefix_group[q];
        cnt[q] = in.hi[q] - in.lo[q];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          cnt[q] = bcnt_add(in.e[q][k].x & g.edge_mask[k][0], cnt[q]);
          cnt[q] = bcnt_add(in.e[q][k].y & g.edge_mask[k][1], cnt[q]);
          cnt[q] = bcnt_add(in.e[q][k].z & g.edge_mask[k][2], cnt[q]);
          cnt[q] = bcnt_add(in.e[q][k].w & g.edge_mask[k][3], cnt[q]);
        }
      }
      const uint32_t row_alt = in.row_alt;
      load_tile(tile + tile_stride < ntiles ? tile + tile_stride : tile, in);  // after the last tile: its own rows once more (cache hits, unused)
      uint32_t alt_mine[P];
      if constexpr (C == P) {
#pragma unroll
        for (int p = 0; p < P; ++p) alt_mine[p] = cnt[p];
      } else {
#pragma unroll
        for (int p = 0; p < P; ++p) alt_mine[p] = p == cg ? cnt[0] : 0u;
      }
      derive_group<P>(A.derived_group, row_alt, alt_mine);
      // (an opaque zero offset per tile: the constants are read from LDS where a site uses them - ds_read_b64 of a wave-uniform address, no VALU
      // slot - instead of being hoisted out of the tile loop into up to 44 VGPRs, which cost the Hudson kernels a wave per SIMD)
      uint32_t ko = 0;
      asm volatile("" : "+v"(ko));
      const double* K = K0 + ko;
      const size_t my_rel = tile * kTileRows + (size_t)lane;
      site_const_epilogue<P, MODE, F, HF>(A, K, my_rel, my_rel < A.row_count, alt_mine, T);
    }
  }
  reduce_block_totals<P, MODE>(A, T);
}

}  // namespace fmh
