/*
 * ferromic_hip.h — C-ABI of libferromic_hip.so: the MI355X (gfx950) device layer under the
 * ferromic per-site diversity / FST hot path.
 *
 * The reference (SauersML/ferromic) has no FFI for this path: PyO3 calls the Rust functions in
 * src/stats.rs directly.  This header is the boundary a Rust (or any) host would bind instead of
 * those functions; every entry point cites the reference code it replaces.  INTEGRATION.md shows
 * the `extern "C"` block a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes; no C++/torch types.  Pointers named d_* are DEVICE pointers
 *     (hipMalloc or a torch tensor's data_ptr), h_* are HOST pointers; every d_* output may be
 *     NULL to skip that track.
 *   - every function returns a status (FMH_OK == 0) and records a thread-local message readable
 *     through fmh_last_error().
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls that fill host
 *     totals synchronise that stream before returning.
 *   - host threads: every function may be called from several threads at once, on one device or several; matrix and groups handles
 *     may be shared by calls that only read them (every statistic), while creating, packing, generating into and destroying a handle
 *     is the business of one thread at a time.  Output buffers belong to one call.  DESIGN.md, "Host threads", lists what the
 *     library serialises internally.
 *   - per-site f64 tracks encode the reference's Option<f64>::None as NaN.
 *   - rows are variant sites in matrix order; a sweep over [row_begin, row_begin+row_count) writes
 *     per-site outputs at index (row - row_begin).
 */
#ifndef FERROMIC_HIP_H
#define FERROMIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMH_ABI_VERSION 3
#define FMH_MAX_GROUPS 8 /* populations per sweep */
#define FMH_MAX_PAIRS 28 /* FMH_MAX_GROUPS choose 2 */

enum fmh_status {
  FMH_OK = 0,
  FMH_ERR_INVALID = 1,     /* bad argument (message says which) */
  FMH_ERR_HIP = 2,         /* HIP runtime error */
  FMH_ERR_NO_DEVICE = 3,   /* no usable GPU: the product path has no CPU fallback */
  FMH_ERR_UNSUPPORTED = 4
};

/* Which of the reference's algebraically-equal formula sets a sweep reproduces bit-for-bit. */
enum fmh_formula {
  /* sparse Variant path: pi_from_components (stats.rs:2723-2733), dxy_from_counts (2907-2935),
   * hudson_site_from_variant (2969-3014), compute_pi_metrics_fast (2761-2821) */
  FMH_FORMULA_SPARSE = 0,
  /* dense matrix path: dense_pi_from_counts (1700-1709), dense_dxy_from_biallelic_counts
   * (1712-1733), dense_hudson_sites_{biallelic,general} (3072-3278), calculate_pi_dense
   * (4434-4597); the no-missing biallelic arms (3218-3273, 4485-4523) are taken automatically
   * when the matrix has no missing mask and max_allele <= 1, exactly as the reference does */
  FMH_FORMULA_DENSE = 1,
  /* build_dense_population_summary (1367-1470): like DENSE but per-site pi is always
   * dense_pi_from_counts (1392, 1409), also on a mask-free matrix */
  FMH_FORMULA_SUMMARY = 2
};

typedef struct fmh_matrix fmh_matrix; /* DenseGenotypeMatrix, stats.rs:250-331 */
typedef struct fmh_groups fmh_groups; /* P column memberships, stats.rs:1246-1295 / 1204-1244 / 1093-1159 */

const char* fmh_last_error(void);
int fmh_abi_version(void);
int fmh_device_count(int* h_count);
/* name, CU count and total memory of a device (for reports) */
int fmh_device_info(int device, char* h_name, size_t name_cap, int* h_compute_units, uint64_t* h_total_mem);

/* ---- options ------------------------------------------------------------------------------------
 * Per-process switches that route kernels or size launches (tests, measurements, and the two a deployment may want:
 * FMH_LAYOUT and FMH_COMM_TRANSPORT).  Keys are the names of the environment variables of the same meaning; the FMH_*
 * environment is read ONCE, when the library first needs an option, and never again - nothing on a launch path calls
 * getenv - so a later change goes through fmh_set_option (value NULL = back to what the process
 * started with: the environment's value, else the default; integers, or the words listed):
 *   FMH_LAYOUT (bytes | packed)   FMH_MASK_MODE (1 | 2)   FMH_DEFER_TILES (1..16)   FMH_PACKED_LPR (4 | 16)   FMH_PACKED_UNROLL
 *   FMH_PACKED_NO_PREFETCH   FMH_COUNTS_MFMA (1 | 2)   FMH_GRID_PER_CU   FMH_GRID_BLOCKS   FMH_MAX_OCC   FMH_UNROLL   FMH_PITCH_ALIGN
 *   FMH_COMM_TRANSPORT (host | rccl)   FMH_UPLOAD_THREADS   FMH_PD_TWO_PLANES   FMH_PD_INT8   FMH_PD_PLANES_BYTES   FMH_PD_KCHUNK
 *   FMH_PD_SB   FMH_PD_OCC   FMH_PIPE   FMH_GRAPH   FMH_ROW_HI (0 | 1 | 2)   FMH_COLUMN_WINDOW (0 | 1 | 2)
 *   FMH_TILED_PLANES (0 | 1 | 2)   FMH_TILED_BYTES   FMH_TILED (-1 | 0 | 1)   FMH_TILED_BATCH (10 | 5 | 2)
 *   FMH_SFS_ITEM_ROWS   FMH_SFS_LDS_BINS   FMH_HAP_THREADS (64 | 256 | 512 | 1024)   FMH_FSTAT_ITEM_ROWS   FMH_FSTAT_LDS_MASK_BYTES
 *   FMH_KIN_BUDGET_BYTES   FMH_QC_ITEM_ROWS   FMH_ASSOC_ITEM_ROWS   FMH_ASSOC_BUDGET_BYTES   FMH_SCORE_ITEM_ROWS   FMH_SCORE_BUDGET_BYTES
 *   FMH_ROH_ITEM_ROWS   FMH_IBD_ITEM_ROWS   FMH_IBD_BUDGET_BYTES   FMH_LMM_ITEM_ROWS   FMH_ADMIX_ITEM_ROWS   FMH_ADMIX_BUDGET_BYTES
 * Values are atomics: setting one while another thread launches is safe (that launch sees the old or the new value). */
int fmh_set_option(const char* key, const char* value_or_null);
int fmh_get_option(const char* key, long long* h_value);

/* ---- raw device memory helpers for hosts that do not bring their own allocator --------------- */
int fmh_device_alloc(int device, size_t bytes, void** d_out);
/* Blocks are recycled through a pool without stream ordering: the caller's outstanding stream work on the block must be
 * complete (every fmh_* call that fills host totals has synchronised its stream; fmh_device_zero has not). */
int fmh_device_free(int device, void* d_ptr);
/* `stream` arguments throughout this header are hipStream_t handles passed as void*.  NULL is HIP's legacy default stream: ordered against
 * every blocking stream of the device - which is what a host that also enqueues work of its own on the default stream wants, and a
 * device-wide serialisation point when several host threads use one GPU.  FMH_STREAM_PER_THREAD is the calling thread's own stream
 * (hipStreamPerThread): not ordered against the default stream or other threads.  run_vcf's region workers pass it to the copies of
 * results that a synchronous fmh_* call has already completed. */
#define FMH_STREAM_PER_THREAD ((void*)2)
int fmh_copy_to_host(int device, void* h_dst, const void* d_src, size_t bytes, void* stream);
int fmh_copy_to_device(int device, void* d_dst, const void* h_src, size_t bytes, void* stream);
/* zero-fills device memory, stream-ordered (no synchronisation): accumulators such as fmh_pairwise_differences' outputs */
int fmh_device_zero(int device, void* d_ptr, size_t bytes, void* stream);
int fmh_stream_synchronize(int device, void* stream);
/* Frees the scratch the library keeps between calls on `device` (the sample-major planes of
 * fmh_pairwise_differences and fmh_kinship_counts, up to 8 GiB; the idle blocks of the pool; the pinned upload staging); it is
 * re-created on demand.  It may be called while other threads' fmh_* calls are in flight on the device and changes none of their
 * results: it waits for a running fmh_pairwise_differences / fmh_kinship_counts (they hold the lock of that scratch for their whole
 * length) and for a running upload, and it frees only pool blocks nobody holds.  (hipFree waits for the device: a slow call, not one
 * for a hot path.) */
int fmh_device_release_scratch(int device);

/* ---- genotype matrix (replaces DenseGenotypeMatrix::new, stats.rs:261-296) ------------------- */
/*
 * Upload a site-major matrix in the reference's host layout: data[site*stride + sample*ploidy + side],
 * stride = samples*ploidy (stats.rs:293); optional missing bitset, one bit per linear entry,
 * LSB-first in u64 words (stats.rs:1298-1302; lib.rs:1188-1189).
 * Resident layout: with max_allele <= 7 (every biallelic and every SNP cohort) the matrix is kept BIT-PACKED - one bit
 * plane per allele bit (1, 2 or 3) plus one "called" plane, 128 columns per 16-byte vector - and the sweeps read 1/8 (1/4 with
 * alleles 2..3, 3/8 with 4..7) of the bytes the u8 layout would cost; the rows are packed on the host (threads, SSE2) into pinned
 * staging, so that only the planes cross PCIe.  Other matrices
 * (max_allele > 7, rows beyond 600 000 columns, FMH_LAYOUT=bytes) keep the u8 rows, padded to a 16-byte pitch, with the
 * missing bitset re-laid as one "called" bit-row per site.  A called value above max_allele is a caller error: the packed
 * layout would lose its high bits, so fmh_matrix_create (while it packs the rows on the host) and fmh_matrix_pack (on the
 * device) detect it and return FMH_ERR_INVALID; the u8 layout keeps the bytes as they are and only uses max_allele as a
 * loop bound.  fmh_matrix_create_packed takes the caller's planes at their word.
 */
int fmh_matrix_create(const uint8_t* h_data, const uint64_t* h_missing_or_null, size_t variants,
                      size_t samples, size_t ploidy, uint8_t max_allele, int device, fmh_matrix** out);
/*
 * The same for a host that already holds BIT PLANES (run_vcf after ingest, a cohort stored packed): plane k = bit k of the allele
 * value (h_plane1 iff max_allele >= 2, h_plane2 iff max_allele >= 4), h_called_or_null = 1 bits for called entries; a row is
 * h_pitch bytes, column c is bit (c & 7) of byte (c >> 3), bits past the last column zero.  No conversion: ceil(H / 8) bytes per site
 * and plane cross PCIe.  With h_pitch = the device's own plane pitch - ceil(H / 8) rounded up to 16 - each plane goes up in ONE copy
 * (then the padding bytes of a row must be zero as well); any other pitch takes a pitched copy, a descriptor per row, which is slow for
 * millions of short rows.  The planes are taken at their word (no max_allele check is possible).
 */
int fmh_matrix_create_packed(const uint8_t* h_plane0, const uint8_t* h_plane1_or_null, const uint8_t* h_plane2_or_null,
                             const uint8_t* h_called_or_null, size_t h_pitch, size_t variants, size_t samples, size_t ploidy,
                             uint8_t max_allele, int device, fmh_matrix** out);
/* Allocate an uninitialised device matrix (filled by fmh_matrix_generate or by the caller). */
int fmh_matrix_alloc(size_t variants, size_t samples, size_t ploidy, int with_missing, uint8_t max_allele,
                     int device, fmh_matrix** out);
/* Wrap caller-owned device memory (e.g. a torch uint8 tensor): d_data rows of `pitch` bytes
 * (pitch % 16 == 0, pitch >= samples*ploidy); d_called_bits_or_null rows of `bits_pitch` bytes
 * (bit h of a row set = entry h is called; bits_pitch % 4 == 0, 4-byte aligned). The wrapper never frees them and never writes
 * them.  The bytes and the called bits of a row past its last column, and the byte under an uncalled entry, may hold anything: neither
 * fmh_matrix_pack nor a sweep, fmh_pairwise_differences or the PCA calls on the u8 rows count them. */
int fmh_matrix_wrap(void* d_data, size_t pitch, void* d_called_bits_or_null, size_t bits_pitch,
                    size_t variants, size_t samples, size_t ploidy, uint8_t max_allele, int device,
                    fmh_matrix** out);
/* Build the bit-packed image of a matrix that holds u8 rows (fmh_matrix_alloc + fmh_matrix_generate, fmh_matrix_wrap);
 * the sweeps use it from then on.  release_bytes != 0 frees the u8 rows of a matrix the library owns (a wrapped matrix
 * keeps the caller's memory).  FMH_ERR_UNSUPPORTED when max_allele > 7 or the rows are too wide; a no-op when the
 * matrix is already packed and holds no bytes. */
int fmh_matrix_pack(fmh_matrix* m, int release_bytes);
int fmh_matrix_destroy(fmh_matrix* m);
/* geometry: any pointer may be NULL */
int fmh_matrix_info(const fmh_matrix* m, size_t* variants, size_t* samples, size_t* ploidy, size_t* pitch,
                    size_t* bits_pitch, int* has_missing, uint8_t* max_allele, int* device);
/* the u8 rows and called bit-rows; NULL for a matrix that holds only its packed image */
int fmh_matrix_device_ptrs(const fmh_matrix* m, void** d_data, void** d_called_bits);
/* Copy back in the reference host layout (tests / oracle). h_missing_or_null must hold
 * ceil(variants*stride/64) words when the matrix has a mask.  The byte of a MISSING entry is 0 whichever route built the
 * matrix (the planes of a missing entry are masked with the called plane on the way out). */
int fmh_matrix_download(const fmh_matrix* m, uint8_t* h_data, uint64_t* h_missing_or_null);
/* max over called entries, computed on the device (what from_variants computes at stats.rs:490) */
int fmh_matrix_scan_max_allele(const fmh_matrix* m, uint8_t* h_max, void* stream);

/*
 * Counter-based synthetic cohort written straight into HBM (bench + parity at sizes no host could
 * hold): entry (site, column) = 1 iff hash24(seed, global_site, column) < threshold[pop_of_column][site],
 * and is missing iff hash24(seed ^ K, global_site, column) < missing_threshold24.  `h_thresholds24` is
 * [n_pops][variants] (values in [0, 2^24]); `h_pop_of_column` is [samples*ploidy] with entries < n_pops.
 * `first_global_site` lets a rank generate its slab of a larger cohort.  oracle/dense_oracle.c holds
 * the identical generator so CPU and GPU see the same matrix without moving it.
 */
int fmh_matrix_generate(fmh_matrix* m, uint64_t seed, uint64_t first_global_site,
                        const uint32_t* h_thresholds24, const uint8_t* h_pop_of_column, int n_pops,
                        uint32_t missing_threshold24, void* stream);

/* ---- memberships --------------------------------------------------------------------------- */
/*
 * P populations as 0/1 column masks, h_column_mask[p*H + h], H = samples*ploidy.  A mask is what
 * DenseMembership::build (stats.rs:1252-1284) / HapMembership::build (1212-1238) reduce a
 * (sample, side) list to: duplicates collapse, out-of-range samples are dropped, the Right side is
 * dropped when ploidy <= 1.  Populations may overlap.  1 <= P <= FMH_MAX_GROUPS.
 * Row width: a packed matrix is swept with bit masks in LDS (P_padded * H / 8 bytes <= 150 KiB, P_padded = 1, 2, 4, 8);
 * on u8 rows the masks sit in LDS as bytes while P_padded * round_up(H, 1024) <= 150 KiB, as bits up to 8x that width,
 * and in global memory beyond (one or two groups at a time) — fmh_population_summaries and fmh_wc_sweep re-batch their
 * groups by themselves, fmh_hudson_sweep / fmh_diversity_sites need no batching.
 */
int fmh_groups_create(const fmh_matrix* m, const uint8_t* h_column_mask, int n_groups, fmh_groups** out);
int fmh_groups_destroy(fmh_groups* g);
int fmh_groups_sizes(const fmh_groups* g, int* n_groups, uint64_t* h_sizes /* [n_groups] mask popcounts */);

/* Host only: what the next sweep of `mode` over these groups reads of every row of a packed matrix - the 16-byte vectors (128 columns each)
 * [*first_vec, *first_vec + *n_vec) of bit plane 0 - and the group whose counts it derives from the matrix's row totals instead of counting
 * (-1: none).  A sweep skips the vectors none of its groups has a member in; on a biallelic matrix with nothing missing whose one or two groups
 * partition the columns it also skips one group's vectors (FMH_COLUMN_WINDOW: 0 = never, 1 = default, row totals kept for matrices of at
 * least 4 096 rows, 2 = at any size).  Every other matrix: the whole row and -1.  Results never depend on the window. */
#define FMH_SWEEP_SUMMARY 1   /* fmh_population_summaries */
#define FMH_SWEEP_HUDSON 3    /* fmh_hudson_sweep */
#define FMH_SWEEP_DIVERSITY 5 /* fmh_diversity_sites */
#define FMH_SWEEP_REGION 7    /* fmh_pair_region_sweep */
#define FMH_SWEEP_WC 8        /* fmh_wc_sweep */
int fmh_sweep_window(const fmh_matrix* m, const fmh_groups* g, int mode, uint32_t* first_vec, uint32_t* n_vec, int* derived_group);

/* Host only: whether the next sweep of `mode` over these groups reads its window from the TILE-TRANSPOSED image of bit plane 0 (*tiled = 1) and
 * the size of that image (*image_bytes, 0 when the matrix holds none).  The image stores the 16 bytes of row r, vector v at byte
 * (((r >> 6) * vectors_per_row + v) * 64 + (r & 63)) * 16, so the 64 rows of a tile share the 128-byte lines of one vector column and a column
 * window is read without a byte the sweep does not need.  It is built wherever the planes of a biallelic matrix with nothing missing are written,
 * and it DOUBLES the resident planes of that matrix (6.4 GB at 10 M sites x 5 000 haplotypes).  FMH_TILED_PLANES: 0 = never built, 1 = default:
 * matrices of at least 4 096 rows whose image fits under FMH_TILED_BYTES (default 16 GiB) and leaves as much again free on the device, 2 = at any
 * size without the free-memory test; a negative FMH_TILED_BYTES is an error.  Without an image every sweep takes the row-major routes.  One or
 * two groups, every sweep but W&C.  FMH_TILED: -1 = default: the tiled route where the window (fmh_sweep_window) is at most 7/8 of the row, 0 = the
 * row-major routes with the image present, 1 = the tiled route wherever it is built.  Per-site results never depend on the route; regional f64
 * sums are the same bits at equal grids and agree within 1e-9 otherwise (the routes differ in occupancy, hence in their default grids). */
int fmh_sweep_tiled(const fmh_matrix* m, const fmh_groups* g, int mode, int* tiled, size_t* image_bytes);

/* Host only: whether the next sweep of `mode` over these groups answers its counted groups from the PREFIX COUNTS of bit plane 0 (*uses_table = 1),
 * how many 16-byte plane vectors per row it still reads (*vectors_read: with the table the groups' partial edge vectors, at most two per counted
 * group and possibly none; without it the window's vectors, fmh_sweep_window's n_vec), and the size of the table (*table_bytes, 0 when the matrix
 * holds none).  The table stores, for every row and every vector boundary b = 0 .. vectors_per_row, the alt count of the row's columns before
 * 128 b as a u16 at byte ((tile * (vectors_per_row + 1) + b) * 64 + (r & 63)) * 2 with tile = r >> 6; it is built beside the tile-transposed image,
 * under that image's rules, on rows of at most 65 535 columns, and costs 2 * (vectors_per_row + 1) bytes per row.  A group whose members are exactly
 * one column range [c0, c1) is then the difference of two entries plus the masked counts of the vectors that hold c0 and c1 when those are not
 * multiples of 128 - integers, so per-site results and regional sums are the bits of the window's.  The table form is taken on the tiled route
 * (fmh_sweep_tiled) when EVERY counted group is such a range; the derived group (fmh_sweep_window) is chosen as without the table and is still not
 * counted.  FMH_PREFIX_COUNTS: 0 = no table is built and none is read, 1 = default: matrices of at least 4 096 rows while as much again stays free on
 * the device, 2 = beside the image at any size without the free-memory test. */
int fmh_sweep_prefix(const fmh_matrix* m, const fmh_groups* g, int mode, int* uses_table, uint32_t* vectors_read, size_t* table_bytes);

/* ---- per-population summary sweep ------------------------------------------------------------ */
typedef struct {
  uint64_t haplotype_capacity; /* mask popcount — DensePopulationSummary.haplotype_capacity (1466) */
  uint64_t segregating_sites;  /* sites with >= 2 distinct called alleles inside the population
                                  (== called>=2 && 0<alt<called when biallelic: 1389, 4049, 3891-4026, 3868-3889) */
  uint64_t uncallable_sites;   /* sites with called < 2 (1512-1516, 4391-4393, 4464, 4586) */
  double pi_sum;               /* sum of per-site pi over sites with called >= 2 (1392-1394, 4388-4390, ...) */
} fmh_pop_totals;

/*
 * Replaces build_dense_population_summary (stats.rs:1367-1470) for all P populations in ONE pass,
 * and supplies the scalars count_segregating_sites_dense (3891), calculate_pi_dense (4534),
 * calculate_pi (4317) and count_segregating_sites_for_haplotypes (3858) reduce to.
 * d_alt / d_called: [P][row_count] u32 (alt = number of allele-1 calls; meaningful when max_allele <= 1).
 */
int fmh_population_summaries(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                             int formula, uint32_t* d_alt, uint32_t* d_called, fmh_pop_totals* h_totals,
                             void* stream);

/* ---- Hudson pair sweep (groups 0 and 1 of `g`) ----------------------------------------------- */
typedef struct {
  /* HudsonSummaryTotals, stats.rs:1545-1552, from aggregate_hudson_components_from_summaries
   * (1554-1623).  Only meaningful when max_allele <= 1. */
  double numerator_sum, denominator_sum, pi1_sum, pi2_sum, dxy_sum_all;
  uint64_t dxy_uncallable_sites;
  /* hudson_component_sums over the per-site records (stats.rs:1625-1635) */
  double site_num_sum, site_den_sum;
  uint64_t sites_with_components;
  /* sum of per-site d_xy over sites where it is Some, and the count where it is None
   * (calculate_d_xy_hudson sparse fold 2476-2496; calculate_dxy_dense 2546-2596) */
  double site_dxy_sum;
  uint64_t site_dxy_skipped;
  fmh_pop_totals pop[2];
} fmh_hudson_totals;

typedef struct { /* SiteFstHudson as structure-of-arrays, stats.rs:536-555; all nullable */
  double* d_fst;
  double* d_dxy;
  double* d_pi1;
  double* d_pi2;
  double* d_num;
  double* d_den;
  uint32_t* d_alt;    /* [2][row_count] */
  uint32_t* d_called; /* [2][row_count]  (n1_called, n2_called) */
} fmh_hudson_sites;

/*
 * One pass over the rows yields what the reference computes in up to four passes:
 * build_dense_population_summary x2 (1367), aggregate_hudson_components_from_summaries (1554),
 * dense_hudson_sites (3060) or hudson_site_from_variant per site (2969), and the pi/Dxy auxiliaries
 * of calculate_hudson_fst_for_pair_core (3435-3599).  This is the "pi + Hudson FST" sweep
 * BASELINE.json's metric is quoted on.
 */
int fmh_hudson_sweep(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                     int formula, const fmh_hudson_sites* sites_or_null, fmh_hudson_totals* h_totals,
                     void* stream);

/*
 * The same Hudson totals and per-site records from the two populations' per-site COUNT TABLES (d_called / d_alt as fmh_population_summaries
 * writes them, biallelic) instead of a matrix: aggregate_hudson_components_from_summaries (stats.rs:1554-1623) takes two
 * DensePopulationSummary objects that need not come from one matrix - ferromic.hudson_fst / hudson_dxy of two Population.from_numpy
 * objects.  capacity1/2 = haplotype_capacity of the two populations (copied into h_totals->pop[]); any_missing != 0 when either matrix
 * has missing calls (selects the kernel twin the fused sweep would have taken; it matters to FMH_FORMULA_DENSE only).  Same per-site code as
 * fmh_hudson_sweep after the counting: the per-site values are its bits, the regional sums differ in the order of their additions.
 */
int fmh_hudson_from_counts(int device, const uint32_t* d_called1, const uint32_t* d_alt1, uint64_t capacity1, const uint32_t* d_called2,
                           const uint32_t* d_alt2, uint64_t capacity2, size_t row_count, int formula, int any_missing,
                           const fmh_hudson_sites* sites_or_null, fmh_hudson_totals* h_totals, void* stream);

/* ---- per-site diversity (population 0 of `g`) ------------------------------------------------- */
/*
 * Replaces the loop of calculate_per_site_diversity (stats.rs:4693-4750): d_pi / d_theta per site;
 * called < 2 -> (NaN, NaN); theta = 1/H_{called-1} when >= 2 distinct alleles else 0 (4717-4722),
 * with H_k summed ascending exactly like harmonic() (4234-4240).  Position filtering / masking
 * (4731-4743) stays on the host.
 */
int fmh_diversity_sites(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                        double* d_pi, double* d_theta, uint32_t* d_called, uint32_t* d_distinct,
                        fmh_pop_totals* h_totals, void* stream);

/* ---- fused region sweep: summaries + per-site diversity of groups 0 and 1 (+ the Hudson pair) in ONE read ---------------------- */
typedef struct { /* calculate_per_site_diversity's SiteDiversity (stats.rs:185-190) of BOTH groups; nullable */
  double* d_pi;    /* [2][row_count] */
  double* d_theta; /* [2][row_count] */
} fmh_pair_diversity_sites;
/*
 * What the reference's region driver (process.rs:2468-3653) computes for haplotype groups 0 and 1 of one variant set in separate walks -
 * process_variants per group (segregating sites, pi: calculate_pi_for_population 4599-4614; per-site diversity: 4628-4806) and the
 * Hudson pair (calculate_hudson_fst_for_pair_with_sites 3619-3625) - from one pass over the matrix:
 *   h_totals->pop[0..1]  the population summaries by `summary_formula`
 *   diversity            per-site pi / theta of both groups (always the sparse formulas, as the reference)
 *   hudson_formula >= 0  per-site Hudson records into `sites` and the Hudson totals by THAT formula set (the driver uses
 *                        FMH_FORMULA_DENSE for the regional pi of a diploid dense matrix and FMH_FORMULA_SPARSE for Hudson);
 *   hudson_formula  < 0  no Hudson part (h_totals' Hudson fields are zero; sites->d_alt / d_called are still written when given).
 * Every value is the bits of the separate calls (same kernel code after the counts); fmh_population_summaries + 2 x fmh_diversity_sites +
 * fmh_hudson_sweep read the matrix four times, this reads it once.
 */
int fmh_pair_region_sweep(const fmh_matrix* m, const fmh_groups* g /* exactly 2 groups */, size_t row_begin, size_t row_count,
                          int summary_formula, int hudson_formula_or_negative, const fmh_pair_diversity_sites* diversity_or_null,
                          const fmh_hudson_sites* sites_or_null, fmh_hudson_totals* h_totals, void* stream);

/* ---- Weir & Cockerham sweep -------------------------------------------------------------------- */
enum fmh_wc_state { /* FstEstimate variants, stats.rs:37-126 */
  FMH_WC_CALCULABLE = 0,
  FMH_WC_INDETERMINATE = 1,
  FMH_WC_NO_VARIANCE = 2,
  FMH_WC_INSUFFICIENT = 3
};

typedef struct {
  /* slot 0 = overall, slot 1+k = pair k in (0,1),(0,2),...,(P-2,P-1) order (stats.rs:1133-1142) */
  double sum_a[1 + FMH_MAX_PAIRS];
  double sum_b[1 + FMH_MAX_PAIRS];
  uint64_t informative_sites[1 + FMH_MAX_PAIRS]; /* sites whose per-site state != insufficient (2172-2203) */
  uint64_t sites_attempted;                      /* rows swept */
} fmh_wc_totals;

/*
 * Replaces calculate_fst_wc_at_site_with_membership (stats.rs:1814-2032) per row and the sums of
 * calculate_overall_fst_wc (2145-2374).  Groups are the sorted labels of SubpopulationMembership
 * (1104-1150).  Per-site outputs, all [(1+npairs)][row_count]: a, b (summed over every allele
 * present at the site, 1859-1985) and the FstEstimate state code; d_group_called [P][row_count]
 * are the population_sizes (1919-1923).  Alleles are discovered over ALL columns of the row
 * (1826-1837), not only grouped ones.
 */
int fmh_wc_sweep(const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                 double* d_a, double* d_b, uint8_t* d_state, uint32_t* d_group_called,
                 fmh_wc_totals* h_totals, void* stream);

/*
 * The same statistics for ANY number of groups (2 <= n_groups <= FMH_MAX_GROUPS_MANY; labels are u8 in the
 * reference, so 256 covers every input).  h_column_mask is a HOST array [n_groups][columns] of 0/1 bytes in
 * sorted-label order.  Counting runs as summary sweeps over batches of 8 groups, the per-site W&C arithmetic
 * in a counts kernel with the same operand order as fmh_wc_sweep (bit-identical per-site a, b).  Device outputs
 * are [(1 + n_groups(n_groups-1)/2)][row_count] (a, b, state; any may be NULL) and [n_groups][row_count]
 * (d_group_called, may be NULL); host outputs h_sum_a / h_sum_b / h_informative_sites have 1 + npairs entries.
 */
#define FMH_MAX_GROUPS_MANY 256
int fmh_wc_sweep_many(const fmh_matrix* m, const uint8_t* h_column_mask, int n_groups, size_t row_begin,
                      size_t row_count, double* d_a, double* d_b, uint8_t* d_state, uint32_t* d_group_called,
                      double* h_sum_a, double* h_sum_b, uint64_t* h_informative_sites, void* stream);

/* ---- pairwise differences ------------------------------------------------------------------------- */
/*
 * Replaces the nested sample-pair loops of calculate_pairwise_differences (stats.rs:4158-4221) for the first
 * n_samples samples of the matrix (sparse model: a genotype is Some iff its first allele is called, and ends
 * at its first missing allele).  Row-major [n_samples][n_samples] device outputs, filled for i < j only:
 *   d_diff[i*n + j] = sum over sites where both genotypes are Some of the all-vs-all allele mismatches
 *                     (len_i*len_j - sum_a cnt_i(a)*cnt_j(a)),
 *   d_both[i*n + j] = number of sites where both genotypes are Some
 * (comparable sites = L*h_i*h_j - (variants - both)*h_i*h_j is host arithmetic, stats.rs:4182-4208).
 * The call ADDS into both buffers (several matrices of the same samples can be accumulated): zero them first (fmh_device_zero).  Needs ploidy <= 127 (int8 MFMA operands; ploidy <= 4 runs on FP4 MFMA, equally exact);
 * one allele-count plane per allele value 0..max_allele, a single plane when the matrix is biallelic with nothing missing.
 */
int fmh_pairwise_differences(const fmh_matrix* m, size_t n_samples, unsigned long long* d_diff,
                             unsigned long long* d_both, void* stream);

/* ---- haplotype PCA (src/pca.rs) --------------------------------------------------------------------- */
/*
 * The reference's chromosome PCA - rows are HAPLOTYPES (column sample * 2 + side of a diploid matrix), features the sites that pass
 * its filter - as three calls, so that the Gram can be checked entry by entry, independent of eigenvector conditioning:
 *
 * fmh_pca_scan_sites: what the site filter of compute_chromosome_pca{,_from_dense} (pca.rs:46-203, 205-413) needs, per row of
 *   [row_begin, row_begin + row_count): d_alt_count = called entries whose allele is 1, over all columns; d_flags = FMH_PCA_SITE_UNCALLED
 *   when some entry is not called | FMH_PCA_SITE_HIGH_ALLELE when some called entry is above 1.  A row with flags 0 is complete and
 *   biallelic and its count is the reference's allele_sum.  The decision itself (maf = min(f, 1.0 - f) >= 0.05, f = count / n in f64)
 *   is the caller's, on the host.  Synchronises `stream`.
 *
 * fmh_pca_gram: d_gram[n][n] (n = samples * 2; ploidy must be 2) = Z Z^T / (n - 1), where Z[h][k] is h_set_value[k] when haplotype h
 *   carries allele 1 at row h_kept_rows[k] and h_clear_value[k] otherwise - for the reference's standardisation (pca.rs:579-662) the
 *   caller passes (1 - mean_k) / sd_k and -mean_k / sd_k.  The kept rows must be complete and biallelic (flags 0).  f64 throughout, on
 *   the f64 matrix cores; Z is never materialised (the operands are expanded from one bit per entry).  The result is exactly symmetric
 *   and two calls on the same input give the same bits (split-K partials are summed in a fixed order, no atomics).  Device memory:
 *   n * n * 8 bytes of output (the caller's) plus scratch of 8 bytes per 64 kept sites and haplotype (haplotypes rounded up to 128)
 *   and, when K is split, 128 KiB per (tile, split); the sum must stay within FMH_PCA_BUDGET_BYTES (16 GiB unless set), else
 *   FMH_ERR_UNSUPPORTED.  n < 2 or n_kept == 0: FMH_ERR_INVALID; ploidy != 2: FMH_ERR_UNSUPPORTED.  Scratch comes from the library's
 *   pool (fmh_device_release_scratch).  Synchronises `stream`.
 *
 * fmh_pca_eigen_scores: the n x n symmetric eigenproblem of d_gram (OVERWRITTEN) and pca.rs:751-797: h_eigenvalues[k] = the k-th
 *   largest eigenvalue, h_scores[i * n_components + k] = U[i][k] * sqrt((n - 1) * lambda_k), a column left zero when lambda_k is
 *   numerically zero.  The sign of a column is the solver's.  rocSOLVER's rocsolver_dsyevd on the device, bound at run time (dlopen;
 *   FMH_ROCSOLVER_LIBRARY names a file); option FMH_PCA_EIGEN = host takes a plain Householder + implicit-QL solver on the host, which is
 *   also the fallback when rocSOLVER cannot be loaded (one warning on stderr: it is O(n^3) on one thread); FMH_PCA_EIGEN = rocsolver
 *   makes that an error instead.  The call takes no stream: rocSOLVER runs on the NULL stream and the call synchronises it; one
 *   eigenproblem at a time per device (the cached rocBLAS handle is guarded by a lock).  n <= 46 340.
 *
 * fmh_pca_eigen_host: that host solver alone (no device): h_matrix[n][n] symmetric in, column k = unit eigenvector of h_eigenvalues[k]
 *   out, eigenvalues ascending.
 *
 * Options: FMH_PCA_EIGEN (host | rocsolver | auto)   FMH_PCA_SPLITS (K splits of the Gram; 1 = none, 0 = by the tile count)
 *          FMH_PCA_BUDGET_BYTES
 */
/* efficient_pca::pca::NEAR_ZERO_THRESHOLD (pca.rs:2): below it a standard deviation counts as zero (scale 1) and an eigenvalue yields a
 * zero column.  UNVERIFIED - the crate's source was not available; no kept site and no tested component comes near it. */
#define FMH_PCA_NEAR_ZERO_THRESHOLD 1e-9
#define FMH_PCA_SITE_UNCALLED 1
#define FMH_PCA_SITE_HIGH_ALLELE 2
int fmh_pca_scan_sites(const fmh_matrix* m, size_t row_begin, size_t row_count, uint32_t* d_alt_count, uint8_t* d_flags, void* stream);
int fmh_pca_gram(const fmh_matrix* m, const uint64_t* h_kept_rows, size_t n_kept, const double* h_set_value,
                 const double* h_clear_value, double* d_gram /* n x n, n = samples * 2 */, void* stream);
int fmh_pca_eigen_scores(int device, double* d_gram, size_t n, size_t n_components, double* h_eigenvalues,
                         double* h_scores /* n x n_components, row-major */);
int fmh_pca_eigen_host(double* h_matrix, size_t n, double* h_eigenvalues);

/* ---- linkage disequilibrium (the project's own definition: the reference has no LD code) ---------------------------- */
/*
 * r^2 between a site and the sites that follow it, and LD pruning, from the bit-packed image (one bit per haplotype and row: the
 * haplotype counts of a site pair are popcounts of the AND of two rows).  Columns are the haplotypes of the matrix, restricted to the
 * one group of `g_or_null` when given (mask M; all columns otherwise).  For site i: C_i = called & M, A_i = (allele >= 1) & C_i - the OR
 * of the allele planes, so a multi-allelic site counts "non-reference".  For a pair i < j:
 *   n = |C_i & C_j|   nA = |A_i & C_j|   nB = |A_j & C_i|   nAB = |A_i & A_j|
 *   D = n * nAB - nA * nB                                               (64-bit integers, exact)
 *   r2 = ((double)D * (double)D) / ((double)(nA * (n - nA)) * (double)(nB * (n - nB)))
 * - the squared Pearson correlation of the two indicator vectors over the jointly called columns.  The integer products are formed in
 * 64-bit integers and converted (each is below 2^53 for every row width the packed layout takes), which leaves three roundings and no
 * fused multiply-add: the value can be reproduced bit for bit on a host.  r2 is a quiet NaN when nA * (n - nA) == 0 or
 * nB * (n - nB) == 0: a site that is monomorphic among the jointly called columns, and n == 0.
 *
 * Band addressing: pairs are (i, d), partner j = i + d, 1 <= d <= band; a band buffer is [row_count][band], entry
 * (i - row_begin) * band + (d - 1).  All index arithmetic is 64-bit.
 *
 * fmh_ld_band: rows [row_begin, row_begin + row_count), partners j < partner_end (row_begin + row_count <= partner_end <= variants: the
 *   partners may reach beyond the rows asked for, which is how a caller walks a range in chunks).  Every output is optional.  Entries with
 *   j >= partner_end are WRITTEN: r2 = NaN, counts 0, bit 0.  `over` holds bit (d - 1) & 31 of word (d - 1) >> 5 = r2 > threshold (NaN
 *   never exceeds), whole words, the padding bits of the last word zero.  d_site_n / d_site_alt [row_count] = |C_i| / |A_i|.
 *   One 256-thread workgroup per 64 rows x 64 values of d; no scratch memory and no atomics: two calls give the same bits.
 *   Enqueues on `stream` and synchronises it, as fmh_pairwise_differences does.
 * fmh_ld_prune: forward greedy thinning, deterministic: keep[*] = 1; for i ascending, if keep[i], every j = i + d (1 <= d <= window,
 *   j < row_begin + row_count) with r2(i, j) > threshold gets keep[j] = 0.  A removed site removes nothing.  The band kernel runs with
 *   only `over`, in row chunks whose threshold bits stay within 64 MiB of device scratch from the library's pool (and as much host
 *   memory) - at least 64 rows per chunk - pairs reaching into the next chunk; the rule is applied chunk by chunk on the host, in order.
 *   fmh_ld_prune_chunked is the same with the chunk length given (0 = the 64 MiB rule): what the tests force a chunk boundary with.
 * fmh_ld_prune_bits: the greedy rule alone over the `over` band of one fmh_ld_band call with partner_end = row_begin + row_count
 *   (bits of partners beyond row_count are ignored).  Host only, no device.
 *
 * Refusals, before anything is enqueued: a matrix without a packed image FMH_ERR_UNSUPPORTED (call fmh_matrix_pack first); band / window
 * == 0, row_begin + row_count > partner_end, partner_end > variants, a group handle with n_groups != 1, a NULL output struct, a NaN
 * threshold FMH_ERR_INVALID; no GPU FMH_ERR_NO_DEVICE.  row_count == 0 is FMH_OK.
 */
typedef struct {            /* all nullable; each [row_count][band] except over */
  double*   r2;
  uint32_t* n_ab;
  uint32_t* n_joint;        /* n of the pair */
  uint32_t* over;           /* [row_count][ceil(band/32)]: bit (d-1)&31 of word (d-1)>>5 = r2 > threshold */
} fmh_ld_band_out;

int fmh_ld_band(const fmh_matrix* m, const fmh_groups* g_or_null /* exactly 1 group */, size_t row_begin, size_t row_count,
                size_t partner_end /* j < partner_end <= variants */, size_t band, double threshold,
                const fmh_ld_band_out* d_out, uint32_t* d_site_n_or_null /* |C_i| */, uint32_t* d_site_alt_or_null /* |A_i| */,
                void* stream);
int fmh_ld_prune(const fmh_matrix* m, const fmh_groups* g_or_null, size_t row_begin, size_t row_count, size_t window,
                 double threshold, uint8_t* h_keep /* [row_count] */, void* stream);
int fmh_ld_prune_chunked(const fmh_matrix* m, const fmh_groups* g_or_null, size_t row_begin, size_t row_count, size_t window,
                         double threshold, uint8_t* h_keep /* [row_count] */, size_t chunk_rows /* 0 = by the scratch bound */,
                         void* stream);
int fmh_ld_prune_bits(const uint32_t* h_over, size_t row_count, size_t band, uint8_t* h_keep);   /* host only, no device */

/* ---- site frequency spectra (an addition: the reference has none) ------------------------------------------------------------
 * Counted from the bit-packed image.  A group is a 0/1 column mask with n >= 1 members (fmh_groups).  A row is handled against a group in
 * this order of precedence:
 *   1. multiallelic: some member is called and carries an allele above 1 - not binned, tallied in `multiallelic`;
 *   2. incomplete:   some member is not called - not binned, tallied in `incomplete`;
 *   3. usable:       binned at k = the number of members whose allele is 1, 0 <= k <= n.
 * Bits of the allele planes under uncalled entries are undefined (fmh_matrix_create_packed accepts junk there): every plane is masked with
 * the called plane.  Monomorphic rows land in bins 0 and n.  For every window  sum(bins) + multiallelic + incomplete == rows of the window.
 * Joint spectrum of groups 0 and 1 (they may overlap and differ in size): a row is multiallelic if it is so for either group, otherwise
 * incomplete if it is so for either group, otherwise binned at [k0][k1].  Rows with missing calls are NOT projected down to a smaller
 * sample size; the tallies say how much was left out.
 * Results are integers (u64) and never depend on a route, an option, the grid or the order in which anything ran.
 *
 * fmh_sfs: the 1-D spectra of ONE group over n_windows row ranges [h_windows[2w], h_windows[2w+1]) of the matrix.  Ranges may overlap, be
 *   empty and come in any order; begin <= end <= variants.  d_sfs is [n_windows][n+1] u64 on the matrix's device, zero-filled by the call;
 *   h_skipped [n_windows] or NULL.
 * fmh_sfs_joint: the joint spectrum of EXACTLY two groups over rows [row_begin, row_begin + row_count): d_sfs [n0+1][n1+1] u64,
 *   zero-filled by the call; h_skipped one entry or NULL.
 * Both enqueue on `stream` and synchronise it.  row_count == 0, or all windows empty, is FMH_OK with a zeroed table.
 * Refusals, before any device work, in this order: a NULL matrix, groups, table or windows pointer; a wrong group count (1 / 2); groups
 * that were not made for this matrix; a group with no member; a window outside the matrix or with begin > end; n_windows == 0 - all
 * FMH_ERR_INVALID; a table of more than 2^28 bins, and a matrix without the packed image (call fmh_matrix_pack first) - FMH_ERR_UNSUPPORTED.
 * Options: FMH_SFS_ITEM_ROWS = rows per work item (default 4 096), FMH_SFS_LDS_BINS = cap on the on-chip tile in bins (default 5 116: an
 * eighth of the device's 160 KiB per CU, eight workgroups resident; at most 40 956: all of it, eight waves resident); neither changes a result.
 *
 * fmh_sfs_stats (host only, no device): the statistics of one 1-D spectrum of sample size n (h_sfs has n + 1 entries), S = the sum of
 * bins 1..n-1:
 *   pi_sum = sum_k sfs[k] 2 k (n-k) / (n (n-1))     theta_w_sum = S / a1     theta_h_sum = sum_{0<k<n} sfs[k] 2 k^2 / (n (n-1))
 *   a1 = sum_{i<n} 1/i   a2 = sum_{i<n} 1/i^2   b1 = (n+1) / (3 (n-1))   b2 = 2 (n^2+n+3) / (9 n (n-1))
 *   c1 = b1 - 1/a1   c2 = b2 - (n+2) / (a1 n) + a2 / a1^2   e1 = c1 / a1   e2 = c2 / (a1^2 + a2)
 *   tajima_d = (pi_sum - S/a1) / sqrt(e1 S + e2 S (S-1)),  NaN when S == 0 or n < 4 (at n = 2 and 3 the variance is zero on paper and
 *   rounding noise in f64);  fay_wu_h = pi_sum - theta_h_sum (unnormalised).  n < 2: every f64 field is NaN.  No sum is divided by a
 *   sequence length.
 */
typedef struct { uint64_t multiallelic, incomplete; } fmh_sfs_skipped;

int fmh_sfs(const fmh_matrix* m, const fmh_groups* g /* exactly 1 group */, const uint64_t* h_windows /* [n_windows][2] */, size_t n_windows,
            uint64_t* d_sfs /* [n_windows][n+1] */, fmh_sfs_skipped* h_skipped_or_null /* [n_windows] */, void* stream);
int fmh_sfs_joint(const fmh_matrix* m, const fmh_groups* g /* exactly 2 groups */, size_t row_begin, size_t row_count,
                  uint64_t* d_sfs /* [n0+1][n1+1] */, fmh_sfs_skipped* h_skipped_or_null, void* stream);

typedef struct {
  uint64_t sites, segregating_sites;          /* sum of all bins; sum of bins 1..n-1 */
  double pi_sum, theta_w_sum, theta_h_sum;    /* not divided by any sequence length */
  double tajima_d, fay_wu_h;                  /* fay_wu_h = pi_sum - theta_h_sum (unnormalised) */
} fmh_sfs_stats_out;
int fmh_sfs_stats(const uint64_t* h_sfs, size_t n, fmh_sfs_stats_out* h_out);   /* host only, no device */

/* ---- Patterson f-statistics: f2, f3, f4 from exact moment blocks (an addition: the reference has none) ------------------------
 * The device returns integers only: per block of rows, the sums of the groups' allele counts and of their pairwise products.  Every f2, f3
 * and f4 over a block, biased or unbiased, is a fixed rational function of those sums and of the constant sample sizes, evaluated once on
 * the host (fmh_fstat_f4).
 * GROUPS: G column masks, h_column_mask[g*columns + c], 0/1 bytes on the host (as fmh_wc_sweep_many takes them), 2 <= G <=
 * FMH_FSTAT_MAX_GROUPS.  Every group has n_g >= 1 members; groups may overlap.
 * ROW CLASSIFICATION, against all G groups at once, in this order of precedence (the joint spectrum's rule):
 *   1. multiallelic: a called member of any group carries an allele above 1;
 *   2. incomplete:   a member of any group is not called;
 *   3. usable:       a_g = the members of g whose allele is 1, 0 <= a_g <= n_g.
 * Every allele plane is masked with the called plane (junk under uncalled entries is allowed); columns no group holds never matter.
 * Monomorphic rows are usable.
 * BLOCKS: row ranges [h_blocks[2b], h_blocks[2b+1]); they may overlap, be empty and come in any order.  For each block the call fills a
 * slice of M = 1 + G + G (G + 1) / 2 u64 (fmh_fstat_moment_count):
 *   [0]             usable rows
 *   [1 + g]         sum of a_g over the usable rows
 *   [1 + G + t]     sum of a_i a_j for i <= j, t = i G - i (i - 1) / 2 + (j - i): the upper triangle row-major, diagonal included
 * and the {multiallelic, incomplete} tallies of the block (fmh_sfs_skipped): usable + multiallelic + incomplete == rows of the block.
 * Results never depend on a route, an option, the grid or the order in which anything ran.
 *
 * fmh_fstat_moments: d_moments is [n_blocks][M] u64 on the matrix's device, zero-filled by the call; h_skipped [n_blocks] or NULL.  The call
 *   enqueues on `stream` and synchronises it.  All blocks empty is FMH_OK with a zeroed table.
 * Refusals, before any device work, in this order: a NULL matrix, mask, blocks or table pointer; n_groups outside 2..32; a group with no
 * member; a block outside the matrix or with begin > end; n_blocks == 0 - all FMH_ERR_INVALID; a block with rows * max(n_g)^2 >= 2^63 (a
 * u64 moment could wrap); a matrix without the packed image (call fmh_matrix_pack first) - FMH_ERR_UNSUPPORTED.
 * Options: FMH_FSTAT_ITEM_ROWS = the most rows of a work item (default 4 096; a longer block is cut into equal items); FMH_FSTAT_LDS_MASK_BYTES = the bytes of a workgroup's LDS the groups'
 * mask entries may take (default 8 192, with which eight workgroups still share a compute unit; a set of groups that needs more is read
 * from global memory; 1 forces that).  Neither changes a result.
 *
 * fmh_fstat_f4 (host only, no device): from ONE block's slice and the G sample sizes, the sum over the block's usable rows of the
 * estimator of (p_A - p_B)(p_C - p_D), p_X = a_X / n_X.  Indices may repeat: f2(A,B) = (A,B;A,B), f3(C;A,B) = (C,A;C,B).  With S_XY the
 * product moments
 *   biased sum = S_AC/(nA nC) - S_AD/(nA nD) - S_BC/(nB nC) + S_BD/(nB nD),
 * evaluated as ONE exact 128-bit integer numerator over the common denominator nA nB nC nD and divided once in f64 (a moment is below
 * 2^63, each term's cofactor at most 2^34 with sizes up to 2^17; beyond that the call refuses).  With `unbiased`, every coincidence
 * of indices removes the bias of p_X^2 with  h_X = (n_X S_X - S_XX) / (n_X^2 (n_X - 1)),  S_X the sum of a_X:
 *   -h_A if A == C,  +h_A if A == D,  +h_B if B == C,  -h_B if B == D;
 * each h_X is one exact integer numerator, one exact integer denominator and one division.  The result is NaN if a needed n_X < 2.  No sum
 * is divided by a site count here.  A NULL pointer, n_groups outside 2..32, an index outside 0..n_groups-1 or a size of 0: FMH_ERR_INVALID;
 * a size above 2^17: FMH_ERR_UNSUPPORTED.
 *
 * fmh_block_jackknife (host only, no device): the weighted delete-one-block jackknife (Busing et al. 1999, as ADMIXTOOLS uses it) of
 * theta = sum(num) / sum(den) over n_blocks blocks of weight m_j = h_weight[j] (NULL: m_j = den_j).  Blocks of weight 0 are dropped; g are
 * left, n = sum m_j, and with the sums over those g blocks
 *   theta_(-j) = (sum num - num_j) / (sum den - den_j)        theta_J = g theta - sum_j (1 - m_j / n) theta_(-j)
 *   h_j = n / m_j      tau_j = h_j theta - (h_j - 1) theta_(-j)      var = (1 / g) sum_j (tau_j - theta_J)^2 / (h_j - 1)
 * Output {estimate = theta, jackknife_estimate = theta_J, se = sqrt(var), z = theta / se, blocks = g}; se and z are NaN when g < 2 (and
 * theta_J = theta at g == 1: the one block's factor 1 - m / n is 0), every f64 field is NaN when sum(den) == 0.  A NULL num, den or output pointer, or a negative or non-finite weight: FMH_ERR_INVALID.
 *
 * Out of scope here: Patterson's D normalisation (its denominator is fourth-order in the counts: u64 sums wrap at n = 5 000 after 8 192
 * rows, it needs 128-bit accumulation; f4 and its Z are the admixture test delivered), projection over missing calls, u8-row matrices,
 * sharding over devices (the tables are integers: a caller adds them).
 */
#define FMH_FSTAT_MAX_GROUPS 32
typedef struct { double estimate, jackknife_estimate, se, z; uint64_t blocks; } fmh_jackknife_out;

int fmh_fstat_moments(const fmh_matrix* m, const uint8_t* h_column_mask /* [n_groups][columns] */, int n_groups,
                      const uint64_t* h_blocks /* [n_blocks][2] */, size_t n_blocks, uint64_t* d_moments /* [n_blocks][M] */,
                      fmh_sfs_skipped* h_skipped_or_null /* [n_blocks] */, void* stream);
size_t fmh_fstat_moment_count(int n_groups);   /* M; 0 when n_groups is outside 2..32; needs no device */
int fmh_fstat_f4(const uint64_t* h_moments /* one block: [M] */, const uint64_t* h_sizes /* [n_groups] */, int n_groups,
                 int A, int B, int C, int D, int unbiased, double* h_sum);   /* host only, no device */
int fmh_block_jackknife(const double* h_num, const double* h_den, const double* h_weight_or_null /* NULL = den */, size_t n_blocks,
                        fmh_jackknife_out* h_out);   /* host only, no device */

/* ---- relatedness: KING-robust kinship from exact genotype-class tables (an addition: the reference has none) ---------------------------
 * The matrix must have ploidy 2.  Sample s owns columns 2s and 2s+1.
 * At row r, the genotype of s is CALLED (c_s(r) = 1) iff both entries are called and both alleles are <= 1.  An entry with a bit in an
 * upper allele plane makes that genotype not called.  Nothing else about the row changes, so no row pre-filter is needed and a
 * multi-allelic row still serves the samples that are 0/1 there.
 * The dosage is g_s(r) in {0, 1, 2}.  Indicator rows over the kept rows are: H for g = 1; R for g = 0; A for g = 2; V = R + A; W = R - A.
 * For samples i, j of the selected list, taken over the kept rows, four u64 tables, row-major [n][n]:
 *   both[i][j]     #{c_i and c_j}.  Diagonal: called genotypes of i
 *   het_het[i][j]  H_i . H_j.  Diagonal: het genotypes of i
 *   ibs0[i][j]     R_i . A_j + A_i . R_j.  Diagonal 0
 *   het_hom[i][j]  H_i . V_j.  NOT symmetric: [i][j] is "i het, j hom".  Diagonal 0
 * All four tables are filled for every i, j, both triangles included.  The call ADDS into the caller's buffers, so chromosomes held as
 * separate matrices of the same samples accumulate.  The caller zeroes the buffers first, as for fmh_pairwise_differences.
 *
 * Host estimators come from those integers, with the operation order fixed (the library is built with -ffp-contract=off, so numpy
 * reproduces the values bit for bit):
 *   het_i = het_het + het_hom[i][j], het_j = het_het + het_hom[j][i], m = min(het_i, het_j).
 *   KING-robust kinship (Manichaikul et al. 2010, between-family form):
 *     phi = 0.5 - (double)(het_hom[i][j] + het_hom[j][i] + 4*ibs0) / (double)(4*m).  It is a quiet NaN when m == 0.  On the diagonal this
 *     gives 0.5, or NaN for a sample without a het call.
 *   IBS distance: (double)(het_hom[i][j] + het_hom[j][i] + 2*ibs0) / (double)(2*both).  It is NaN when both == 0.
 *   Unrelated subset (host, deterministic): repeat the following until no remaining pair has phi > threshold.  Count, for every remaining
 *     sample, its remaining partners with phi > threshold.  Remove the sample with the largest count, taking the highest index on a tie.
 *     NaN never exceeds the threshold.  (Partner j of i is read from h_kinship[i][j].)
 *
 * fmh_kinship_counts: samples = h_samples_or_null (ascending, distinct matrix sample numbers) or the first n_samples (a list that is
 *   0 .. n_samples-1 is recognised and handled as NULL: no list is uploaded, the planes kernel copies row pieces instead of gathering); rows = those of
 *   [row_begin, row_begin + row_count) whose h_keep_or_null byte is non-zero (NULL: all of them; the bytes are what fmh_ld_prune writes).
 *   *h_kept_rows (may be NULL) receives the NUMBER of kept rows.  With no kept row the call returns FMH_OK and adds nothing.  The bits of
 *   the allele planes under uncalled entries are undefined: every class is masked with the called plane.  Enqueues on `stream` and
 *   synchronises it.  The tables come from self-Grams of class operand planes (H and V stacked with an all-ones row; W, signed) on the
 *   matrix cores, through the Gram kernels and launcher of fmh_pairwise_differences: FMH_PD_INT8, FMH_PD_PHASED, FMH_PD_SLABS,
 *   FMH_PD_SLAB_BYTES, FMH_PD_PLANES_BYTES and FMH_PD_KCHUNK apply.  W runs as signed FP4 (e2m1 code 0xA = -1) unless FMH_PD_INT8 is set.
 *   Scratch: (2n+1)^2 * 8 + n^2 * 8 bytes (a matrix with a called plane or an upper allele plane) or 2 * n^2 * 8 bytes, from the pool, plus
 *   the planes workspace; more than FMH_KIN_BUDGET_BYTES (default 16 GiB) is refused.
 * Refusals, all before any launch.  FMH_ERR_INVALID: NULL matrix, NULL out or NULL table; n_samples == 0; a sample index out of range, or
 *   the list not strictly ascending; a row range past the matrix.  FMH_ERR_UNSUPPORTED, with a message: ploidy != 2; a matrix without a
 *   packed image (u8 rows only: alleles >= 8, FMH_LAYOUT=bytes; call fmh_matrix_pack first); over budget.
 * fmh_kinship_stats / fmh_kinship_unrelated: NULL argument (h_ibs_distance_or_null excepted) FMH_ERR_INVALID; n == 0 is FMH_OK.
 * Not built: sharding over devices (the tables are plain sums over rows: a caller adds row slabs), run_vcf wiring, u8 rows.
 */
typedef struct { unsigned long long *d_both, *d_het_het, *d_ibs0, *d_het_hom; } fmh_kinship_out;  /* each [n][n], device, ADDED into */
int fmh_kinship_counts(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */,
                       size_t n_samples, size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count], as fmh_ld_prune writes it */,
                       const fmh_kinship_out* out, uint64_t* h_kept_rows /* may be NULL */, void* stream);
int fmh_kinship_stats(const uint64_t* h_both, const uint64_t* h_het_het, const uint64_t* h_ibs0, const uint64_t* h_het_hom, size_t n,
                      double* h_kinship /* [n][n] */, double* h_ibs_distance_or_null);          /* host only, no device */
int fmh_kinship_unrelated(const double* h_kinship, size_t n, double threshold, uint8_t* h_keep);  /* host only, no device */

/* ---- genotype QC: per-site and per-sample genotype class counts, Hardy-Weinberg exact test (an addition: the reference has none) --------
 * The first step of the cohort chain QC -> fmh_ld_prune -> fmh_kinship_counts -> PCA.
 * The matrix must have ploidy 2 and a packed image.  Sample s owns columns 2s and 2s+1.  c_s(r) ("called") and g_s(r) in {0, 1, 2}
 * ("dosage") are fmh_kinship_counts': the genotype of s at row r is called iff both entries are called and both alleles are <= 1.  The bits
 * of the allele planes under uncalled entries are undefined: every class is masked with the called plane.
 * The selected samples are h_samples_or_null (strictly ascending, distinct matrix sample numbers), or the first n_samples when it is NULL;
 * n = n_samples.
 *
 * Site tracks (fmh_genotype_site_out).  For every row of [row_begin, row_begin + row_count) three u32: hom_ref, het, hom_alt = the number of
 *   selected samples with c = 1 and g = 0, 1, 2.  Structure-of-arrays device buffers [row_count], WRITTEN (not added).  The keep mask does
 *   not apply to them: a filter is derived from them.
 * Sample tables (fmh_genotype_sample_out).  For every selected sample, at its position in the list, three u64: hom_ref, het, hom_alt = the
 *   number of rows of the range whose h_keep_or_null byte is non-zero (NULL: every row; the bytes are what fmh_ld_prune writes) at which the
 *   sample has c = 1 and g = 0, 1, 2.  Device buffers [n], ADDED into, as fmh_kinship_counts' tables are: chromosomes held as separate
 *   matrices of the same samples accumulate; the caller zeroes the buffers first.
 * Weighted called sum (optional).  With h_row_weight_or_null (u32 [row_count], any values) the call adds
 *   sum over the kept rows r of w_r * c_s(r)  into d_weighted_called (u64 [n]), exactly.  The per-sample inbreeding coefficient needs the sum
 *   of a real-valued per-site expectation e_r over the sites where the sample is called; the host hands it over as fixed point,
 *   w_r = rint(e_r * 2^31) with e_r in [0, 1] (fmh_genotype_site_weights), so that the device sum stays an exact integer.
 * Every output pointer may be NULL and that output is then not computed: with no site pointer no track is written and no row reduction is
 *   paid for; with no sample pointer no vertical counter is kept.  *h_kept_rows (may be NULL) receives the number of kept rows.  With no
 *   kept row nothing is added to the sample buffers and the call is FMH_OK.  Enqueues on `stream` and synchronises it.
 * Refusals, all before any launch.  FMH_ERR_INVALID: NULL matrix; n_samples == 0; a sample index out of range, or the list not strictly
 *   ascending; a row range past the matrix; every output NULL; row weights without d_weighted_called, or the reverse.  FMH_ERR_UNSUPPORTED,
 *   with a message: ploidy != 2; a matrix without a packed image (u8 rows only: call fmh_matrix_pack first).
 * Option: FMH_QC_ITEM_ROWS = the most rows of a work item (default 4 096).  It changes no result, nor do FMH_GRID_PER_CU and FMH_GRID_BLOCKS.
 *
 * Hardy-Weinberg exact test (Wigginton, Cutler & Abecasis 2005), array-free.  This is the DEFINITION; device, host twin and a plain Python
 * loop over floats agree bit for bit (the library is built with -ffp-contract=off; f64 division and subnormals are IEEE):
 *   N = hom_ref + het + hom_alt.  N == 0: a quiet NaN.
 *   rare = 2 * min(hom_ref, hom_alt) + het, common = 2N - rare.  rare == 0: 1.0.
 *   mid = rare * common / (2N) in u64 integer division, + 1 if its parity differs from rare's.  The relative weight at mid is t = 1.0.
 *   Walking DOWN (x = mid, r = (rare - mid) / 2, c = N - x - r; while x >= 2):
 *     t = (t * (double)(x * (x - 1))) / (double)(4 * (r + 1) * (c + 1)), then x -= 2, r += 1, c += 1: t is the weight at the new x.
 *   Walking UP from mid again with t = 1.0 (while x + 2 <= rare):
 *     t = (t * (double)(4 * r * c)) / (double)((x + 2) * (x + 1)), then x += 2, r -= 1, c -= 1.
 *   The integer products are formed in u64 and converted; they stay below 2^53 while N <= 2^26.
 *   Pass 1: S = the sum of all weights in the order mid, down, up (starting from 0.0); t_obs = the weight at x == het (0.0 if never met).
 *   Pass 2: the same walk; P = the sum, in that order, of the weights with t <= t_obs.
 *   p = P / S, replaced by 1.0 if greater.  A walk stops once t == 0.0: every later term is zero too.
 *   A site with N > 2^26: fmh_hwe_exact_host refuses the call (FMH_ERR_UNSUPPORTED); fmh_hwe_exact, which cannot look before its launch,
 *   writes a quiet NaN there.
 * fmh_hwe_exact: one thread per site, d_p[i] from the three device tracks; enqueues on `stream` and synchronises it.  n_sites == 0 is FMH_OK;
 *   a NULL pointer FMH_ERR_INVALID.  fmh_hwe_exact_host: the same function on host arrays, no device.
 *
 * Host estimators (no device), the operation order fixed; a quiet NaN results where a denominator is 0.
 *   Site (fmh_genotype_site_stats): n_alt = 2 * hom_alt + het, n_ref = 2N - n_alt.
 *     call_rate = (double)N / (double)n_samples      alt_frequency p = (double)n_alt / (double)(2N)      maf = min(p, 1.0 - p)
 *     f_is = 1.0 - (double)(het * (2N - 1)) / (double)(n_alt * n_ref)
 *     expected_het = (double)(n_alt * n_ref) / (double)(2N - 1): the unbiased HWE-expected het COUNT, an integer ratio with one division.
 *   Weights (fmh_genotype_site_weights): e = (double)(n_alt * n_ref) / (double)(N * (2N - 1)), 0.0 where N == 0; w = rint(e * 2^31) as u32
 *     (e <= N / (2N - 1) <= 1, so w <= 2^31).
 *   Sample (fmh_genotype_sample_stats): called = hom_ref + het + hom_alt.
 *     call_rate = (double)called / (double)kept_rows      het_rate = (double)het / (double)called
 *     F = 1.0 - (double)het / ((double)weighted_called / 2^31): PLINK's --het method-of-moments F with the expectation taken over the
 *     sample's own called sites.
 *   Each output pointer of the two _out structs may be NULL.  A site with N >= 2^31 is refused (FMH_ERR_UNSUPPORTED: the products would
 *   leave a u64); a NULL input FMH_ERR_INVALID (h_weighted_called_or_null may be NULL when h_f is); zero sites / samples is FMH_OK.
 * Not built: sharding over devices (the tables are plain sums over rows: a caller adds row slabs), run_vcf wiring, u8 rows, the mid-p and
 *   X-chromosome variants of the test, a `sites` pre-filter argument for fmh_ld_prune.
 */
typedef struct { uint32_t *d_hom_ref, *d_het, *d_hom_alt; } fmh_genotype_site_out;   /* each [row_count], device, written; any may be NULL */
typedef struct { unsigned long long *d_hom_ref, *d_het, *d_hom_alt, *d_weighted_called; } fmh_genotype_sample_out;  /* each [n], device, ADDED into; any may be NULL */
int fmh_genotype_counts(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */,
                        size_t n_samples, size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count], as fmh_ld_prune writes it */,
                        const uint32_t* h_row_weight_or_null /* [row_count] */, const fmh_genotype_site_out* site_or_null,
                        const fmh_genotype_sample_out* sample_or_null, uint64_t* h_kept_rows /* may be NULL */, void* stream);
int fmh_hwe_exact(const uint32_t* d_hom_ref, const uint32_t* d_het, const uint32_t* d_hom_alt, size_t n_sites, double* d_p, int device,
                  void* stream);
int fmh_hwe_exact_host(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites, double* h_p);  /* no device */
typedef struct { double *h_call_rate, *h_alt_frequency, *h_maf, *h_f_is, *h_expected_het; } fmh_genotype_site_stats_out;  /* each [n_sites] or NULL */
int fmh_genotype_site_stats(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites, uint64_t n_samples,
                            const fmh_genotype_site_stats_out* out);   /* host only, no device */
int fmh_genotype_site_weights(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites,
                              uint32_t* h_weight);   /* host only, no device */
typedef struct { double *h_call_rate, *h_het_rate, *h_f; } fmh_genotype_sample_stats_out;  /* each [n] or NULL */
int fmh_genotype_sample_stats(const uint64_t* h_hom_ref, const uint64_t* h_het, const uint64_t* h_hom_alt,
                              const uint64_t* h_weighted_called_or_null, size_t n, uint64_t kept_rows,
                              const fmh_genotype_sample_stats_out* out);   /* host only, no device */

/* ---- association scan: exact fixed-point dosage sums, linear regression per site (an addition: the reference has none) -----------------
 * The consumer of the cohort chain QC -> fmh_ld_prune -> fmh_kinship_counts -> PCA: for every site the regression of each phenotype on the
 * genotype dosage, with an intercept and covariates (typically the principal components) in the model; beta, its standard error, t and p.
 * Matrix, samples and genotype are fmh_genotype_counts': ploidy 2, a packed image, sample s owns columns 2s and 2s+1; c_s(r) = 1 when the
 * genotype of s at row r is called (both entries called and both alleles <= 1), g_s(r) in {0, 1, 2} the dosage.  Bits under uncalled
 * entries are undefined: every class is masked with the called plane.  The selected samples are h_samples_or_null (strictly ascending,
 * distinct matrix sample numbers) or the first n_samples; n = n_samples; i is a position in that list.
 *
 * Device sums (fmh_assoc_sums).  Given V[n][K] (i32, host, row-major by sample), for every row r of [row_begin, row_begin + row_count) and k < K:
 *     S[r][k] = sum_i c_i(r) * g_i(r) * V[i][k]   (dosage sum)        C[r][k] = sum_i c_i(r) * V[i][k]   (called sum; optional output)
 *   Both are exact `long long` device buffers [row_count][K], WRITTEN (not added).  Limits: 1 <= K <= 64, |V| <= 2^30, n <= 2^22, so
 *   |S| <= 2 * 2^22 * 2^30 = 2^53: every sum converts to f64 without rounding.  V travels as four signed base-256 digits (d in [-128, 127])
 *   and the contraction over samples runs on the int8 matrix cores straight from the bit planes; an i32 digit accumulator holds at most
 *   2 * n * 128 <= 2^30.  A matrix that is biallelic with nothing missing needs no second contraction: the call fills C with the column
 *   totals T[k] = sum_i V[i][k].  Enqueues on `stream` and synchronises it.
 *   Refusals, all before any launch, in this order.  FMH_ERR_INVALID: NULL matrix, values or d_dosage_sum; n_samples == 0 or > 2^22; K
 *   outside 1..64; a value beyond +-2^30; a sample index out of range, or a list that is not strictly ascending (n_samples beyond the
 *   matrix's samples without a list); a row range past the matrix.  FMH_ERR_UNSUPPORTED, with a message: ploidy != 2; a matrix without a
 *   packed image (u8 rows only: call fmh_matrix_pack first).  row_count == 0 is FMH_OK.
 *   Option: FMH_ASSOC_ITEM_ROWS = the most rows of a work item (default 4 096).  It changes no result, nor do FMH_GRID_PER_CU and FMH_GRID_BLOCKS.
 *
 * Host preparation (fmh_assoc_prepare, no device).  h_phenotypes f64 [n][P], P >= 1; h_covariates_or_null f64 [n][c_in], both in the order
 * of the selected samples.  The operation order is fixed, so that a plain Python loop over floats reproduces the integers (the library is
 * built with -ffp-contract=off).  A "sequential" sum starts from 0.0 and adds in sample order.
 *   1. Intercept: always in the model and NEVER a value column.  Every covariate and phenotype column is centred: mean = (sequential sum) / n,
 *      then x_i = x_i - mean.  (A constant column 1/sqrt(n) would round every entry the same way, and that systematic error is amplified by
 *      the cancellation in D below.)
 *   2. Covariates, in column order: r0 = sqrt(sequential sum of x_i * x_i) of the centred column.  Then, twice over: for each kept column q in
 *      the order kept, d = sequential sum of q_i * x_i, then x_i = x_i - d * q_i (modified Gram-Schmidt).  r = sqrt(sequential sum of
 *      x_i * x_i).  r0 == 0 or r <= r0 * 2^-26: the column is dropped as constant or collinear (h_dropped_or_null[j] = 1, else 0).
 *      Otherwise x_i = x_i / r and the column is kept; c = the number kept.
 *   3. Phenotypes: centred, then the c kept columns projected off the same way, twice over.
 *   4. Fixed point, per kept column and phenotype: e_k = the largest integer with max_i |v_ik| * 2^e_k <= 2^30 (from frexp: max = f * 2^x with
 *      f in [0.5, 1) gives e = 31 - x when f == 0.5, else 30 - x); e_k = 0 for a column of zeros.
 *   5. Outputs: V[i][k] = (int32) rint(v_ik * 2^e_k) [n][K] with K = c + P, columns 0..c the basis and c..c+P the phenotypes (h_values must
 *      hold n * (c_in + P) entries; n * K are written, row pitch K); e[K]; T[K] exact i64; yy[p] = sequential sum of (V[i][c+p] * 2^-e)^2;
 *      *h_n_basis = c.  h_exponent and h_total hold c_in + P entries.
 *   Refusals (FMH_ERR_INVALID): a NULL pointer (h_dropped_or_null excepted; h_covariates_or_null when c_in == 0); P == 0; n == 0 or
 *   n > 2^22; a non-finite input; n - c - 2 < 1; c + P > 64.
 *
 * Host statistics (fmh_assoc_stats, no device).  Per row: S and C [K], the three u32 QC tracks hom_ref, het, hom_alt of the same rows and
 * samples (fmh_genotype_counts), T, e, yy, n, c, P.  Missing genotypes are mean-imputed (as regenie and fastGWA do):
 *     N = hom_ref + het + hom_alt;  n_alt = het + 2 * hom_alt;  mu = (double)n_alt / (double)N
 *     a_k  = ldexp((double)S_k + mu * (double)(T_k - C_k), -e_k)              k < K   (T_k - C_k in i64)
 *     gg   = (double)(het + 4 * hom_alt) - (double)(n_alt * n_alt) / (double)N         (u64 product)
 *     D    = gg - a_0 * a_0 - a_1 * a_1 - ... - a_{c-1} * a_{c-1}                      (subtracted in that order)
 *     beta = a_{c+p} / D;   rss = yy_p - (a_{c+p} * a_{c+p}) / D, 0.0 if negative;   df = n - c - 2
 *     se   = sqrt((rss / (double)df) / D);   t = beta / se;   p = the two-sided Student-t tail of |t| with df degrees of freedom
 *   N == 0 or not D > 0: a quiet NaN in all four outputs of the row.  se == 0: t and p are NaN.
 *   p = I_x(df/2, 1/2), the regularised incomplete beta function at x = df / (df + t^2), with xc = t^2 / (df + t^2) for 1 - x:
 *     t^2 == 0: 1.0.  x == 0: 0.0.  a = df / 2.0, b = 0.5,
 *     front = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(xc));
 *     x < (a + 1) / (a + b + 2):  p = front * cf(a, b, x) / a;  otherwise  p = 1.0 - front * cf(b, a, xc) / b,
 *     cf the continued fraction by the modified Lentz method (floor 1e-300), iterated until a step changes it by less than 1e-15 relative.
 *   Outputs beta, se, t, p: f64 [rows][P]; each may be NULL.  Refusals (FMH_ERR_INVALID): P == 0; c + P > 64; n > 2^22 or n - c - 2 < 1; a
 *   NULL input with n_rows > 0.  n_rows == 0 is FMH_OK.
 * Not built: per-phenotype missing values (a NaN is refused), dominant / recessive coding, sharding over devices (a caller
 *   splits rows), run_vcf wiring, u8 rows, more than 64 value columns per call.  Case / control phenotypes: the next section.
 */
int fmh_assoc_sums(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                   size_t row_begin, size_t row_count, const int32_t* h_values /* [n_samples][n_columns] */, size_t n_columns,
                   long long* d_dosage_sum /* [row_count][n_columns], device, written */,
                   long long* d_called_sum_or_null /* [row_count][n_columns], device, written */, void* stream);
int fmh_assoc_prepare(const double* h_phenotypes /* [n][n_phenotypes] */, const double* h_covariates_or_null /* [n][n_covariates] */, size_t n,
                      size_t n_phenotypes, size_t n_covariates, int32_t* h_values /* n * (n_covariates + n_phenotypes) entries; [n][K] written */,
                      int32_t* h_exponent, long long* h_total /* n_covariates + n_phenotypes entries each; K written */,
                      double* h_yy /* [n_phenotypes] */, size_t* h_n_basis, uint8_t* h_dropped_or_null /* [n_covariates] */);   /* host only, no device */
int fmh_assoc_stats(const long long* h_dosage_sum, const long long* h_called_sum /* [n_rows][n_basis + n_phenotypes] each */,
                    const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt /* [n_rows] each */, size_t n_rows,
                    const long long* h_total, const int32_t* h_exponent /* [n_basis + n_phenotypes] each */, const double* h_yy /* [n_phenotypes] */,
                    uint64_t n_samples, size_t n_basis, size_t n_phenotypes,
                    double* h_beta, double* h_se, double* h_t, double* h_p /* [n_rows][n_phenotypes] each, or NULL */);   /* host only, no device */

/* ---- logistic association scan: score test from exact class sums (an addition: the reference has none) -----------------------------------
 * The association scan for case / control phenotypes: per site the score test of the genotype dosage in a logistic model with an intercept
 * and covariates, the null model (covariates only) fitted once per phenotype on the host.  Matrix, samples, c_i(r), g_i(r), row ranges and
 * the row tables are fmh_assoc_sums'.  With g~_i = g_i where the genotype is called and mu (the row's mean dosage) where it is not, the
 * statistic of a row needs  sum_i g~_i r_i,  sum_i g~_i b_ij  and  sum_i w_i g~_i^2  for per-sample columns r, b_j, w of the null model.  The
 * first two are S + mu (T - C) of fmh_assoc_sums.  The third is not linear in the dosage: g^2 = g + 2 [g = 2], so it is S + 2 H + mu^2 (T - C)
 * of the w column with H the sum over the hom-alt genotypes.  The device returns integers only; every f64 follows from them in a fixed order.
 *
 * Hom-alt sums (fmh_assoc_homalt_sums).  Given V[n][K] (i32, host, row-major by sample), for every row r of the range and k < K:
 *     H[r][k] = sum_i c_i(r) * [g_i(r) == 2] * V[i][k]
 *   an exact `long long` device buffer [row_count][K], WRITTEN (not added); every entry has one writer.  Limits: 1 <= K <= 64, |V| <= 2^30,
 *   n <= 2^21, so that |S + 2 H| <= 2 * 2^21 * 2^30 + 2 * 2^21 * 2^30 = 2^53 converts to f64 without rounding.  The contraction is
 *   fmh_assoc_sums' (four signed base-256 digits on the int8 matrix cores, straight from the bit planes) with the operand
 *   lo & hi & "both entries called and no upper-plane bit".  Enqueues on `stream` and synchronises it.
 *   Refusals, all before any launch, are fmh_assoc_sums' in its order.  FMH_ERR_INVALID: NULL matrix, values or d_homalt_sum; n_samples == 0
 *   or > 2^21; K outside 1..64; a value beyond +-2^30; a sample index out of range, or a list that is not strictly ascending (n_samples
 *   beyond the matrix's samples without a list); a row range past the matrix.  FMH_ERR_UNSUPPORTED, with a message: ploidy != 2; a matrix
 *   without a packed image.  row_count == 0 is FMH_OK.  Options: FMH_ASSOC_ITEM_ROWS, FMH_GRID_PER_CU and FMH_GRID_BLOCKS govern this call
 *   as they do fmh_assoc_sums, and change no result.
 *
 * Null model (fmh_logistic_null, host, no device).  h_phenotypes f64 [n][P], every entry exactly 0.0 (control) or 1.0 (case);
 * h_covariates_or_null f64 [n][c_in], both in the order of the selected samples.  The operation order is fixed, so that a plain Python loop
 * over floats reproduces every integer (the library is built with -ffp-contract=off; exp, log and erfc are the C library's).  A
 * "sequential" sum starts from 0.0 and adds in ascending index order.
 *   1. Covariates: centred and orthonormalised exactly as fmh_assoc_prepare's steps 1 and 2, with the same drop rule and the same
 *      h_dropped_or_null report; c = the number kept, q_j the kept columns.
 *   2. Design, d = c + 1 columns: x_i0 = 1.0 / sqrt((double)n) for every i, x_ij = q_{j-1}(i) for j = 1 .. c.
 *   3. Null fit of a phenotype y (Newton / IRLS, no step halving).  n_cases = the number of y_i == 1.0.  n_cases == 0 or == n: not fitted,
 *      reason FMH_LOGISTIC_ONE_CLASS, 0 steps.  Start (the intercept-only fit): beta_0 = log((double)n_cases / (double)(n - n_cases)) / x_00,
 *      beta_j = 0.0 otherwise.  Then steps s = 1, 2, .. 25:
 *        a. per sample eta_i = sequential sum over j of x_ij * beta_j;  mu_i = 1.0 / (1.0 + exp(-eta_i));  w_i = mu_i * (1.0 - mu_i).  The first
 *           w_i that is not > 0.0: not fitted, FMH_LOGISTIC_ZERO_WEIGHT (iterations = the steps completed before).
 *        b. gradient g_j = sequential sum over i of x_ij * (y_i - mu_i); Hessian, for k <= j, A_jk = sequential sum over i of (x_ij * w_i) * x_ik.
 *        c. Cholesky A = L L^T: for j = 0 .. c, for k = 0 .. j: s = A_jk, then s = s - L_jm * L_km for m = 0 .. k-1 in that order; k < j:
 *           L_jk = s / L_kk; k == j: s not > 0.0: not fitted, FMH_LOGISTIC_PIVOT; else L_jj = sqrt(s).
 *        d. forward, j = 0 .. c: s = g_j, s = s - L_jm * z_m for m = 0 .. j-1, z_j = s / L_jj.  Backward, j = c .. 0: s = z_j,
 *           s = s - L_mj * delta_m for m = j+1 .. c ascending, delta_j = s / L_jj.
 *        e. beta_j = beta_j + delta_j; iterations = s.  Every |delta_j| finite and the largest < 1e-8: converged - mu and w are recomputed
 *           from the final beta as in a. (a w_i not > 0.0: FMH_LOGISTIC_ZERO_WEIGHT) and the fit ends.
 *      25 steps without convergence: not fitted, FMH_LOGISTIC_NOT_CONVERGED.  (A phenotype that a covariate separates ends in one of the
 *      last three reasons; which one is decided by this order alone.)
 *   4. Whitened basis of a fitted phenotype.  For j = 0 .. c in order: z_i = sqrt(w_i) * x_ij; r0 = sqrt(sequential sum of z_i * z_i); then,
 *      twice over, for each u already kept, in the order kept: t = sequential sum of u_i * z_i, z_i = z_i - t * u_i; r = sqrt(sequential sum
 *      of z_i * z_i); r0 == 0 or r <= r0 * 2^-26: not fitted, FMH_LOGISTIC_BASIS_LOST; else u_j(i) = z_i / r.  (No centring here.)
 *   5. Value columns of phenotype p, W = c + 3 of them: b_j(i) = sqrt(w_i) * u_j(i) for j = 0 .. c; then r_i = y_i - mu_i; then w_i.  Each is
 *      turned into i32 fixed point with its exponent and exact i64 total by fmh_assoc_prepare's step 4.  A phenotype that is not fitted has
 *      zeros in all W columns, exponents and totals.
 *   6. Layout.  B = floor(64 / W) phenotypes form a batch; batch t holds phenotypes tB .. min(P, tB + B) - 1, Pb of them.  Its values are
 *      one [n][Pb * W] i32 table (row-major by sample, phenotype after phenotype within a row) at h_values + n * W * B * t: exactly the
 *      h_values / n_columns = Pb * W of one fmh_assoc_sums call.  h_exponent and h_total are [P][W]; those of batch t start at entry W * B * t.
 *      h_values must hold n * P * (c_in + 3) entries, h_exponent and h_total P * (c_in + 3); n * P * W and P * W are written.
 *      Per phenotype: h_fitted (1 / 0), h_reason (FMH_LOGISTIC_*), h_iterations, h_n_cases.  *h_n_basis = c.
 *   Refusals (FMH_ERR_INVALID): a NULL pointer (h_dropped_or_null excepted; h_covariates_or_null when c_in == 0); P == 0; n == 0 or
 *   n > 2^21; a non-finite covariate; a phenotype entry other than 0.0 or 1.0; c + 3 > 64; n < c + 3.
 *
 * Score and variance (fmh_logistic_score on the device, fmh_logistic_score_host its twin; ONE function compiled for both, bitwise equal).
 * For one batch of Pb phenotypes, K = Pb * W: S, C [rows][K] from fmh_assoc_sums on the batch's values; H [rows][Pb] from
 * fmh_assoc_homalt_sums on the batch's Pb w columns ([n][Pb]); the three u32 QC tracks of the same rows and samples; T[K], e[K]; c; Pb.
 * Missing genotypes are mean-imputed, as in the linear scan.  Per row:
 *     N = hom_ref + het + hom_alt;  n_alt = het + 2 * hom_alt;  mu = (double)n_alt / (double)N
 *   and per phenotype p, with o = p * W  (T_k - C_k and S_k + 2 H_p in i64):
 *     a_j = ldexp((double)S[o+j] + mu * (double)(T[o+j] - C[o+j]), -e[o+j])                                   j = 0 .. c
 *     U   = the same expression at column o + c + 1
 *     qq  = ldexp((double)(S[o+c+2] + 2 * H[p]) + (mu * mu) * (double)(T[o+c+2] - C[o+c+2]), -e[o+c+2])
 *     Vr  = qq - a_0 * a_0 - a_1 * a_1 - ... - a_c * a_c                                                      (subtracted in that order)
 *   score[r][p] = U, variance[r][p] = Vr: f64 [rows][Pb], WRITTEN.  N == 0, n_alt == 0 or n_alt == 2N (a site without variation carries no
 *   test; an integer rule): a quiet NaN in both.  fmh_logistic_score runs one thread per (row, phenotype) with 64-bit indices, uploads T and
 *   e, enqueues on `stream` and synchronises it.
 *   Refusals: FMH_ERR_INVALID for Pb == 0 or Pb * (c + 3) > 64, then - unless n_rows == 0, which is FMH_OK - for a NULL pointer;
 *   FMH_ERR_UNSUPPORTED for more than 2^39 (row, phenotype) pairs in one device call.
 *
 * Statistics (fmh_logistic_stats, host, no device).  Per entry of U and Vr:
 *     chi2 = U * U / Vr      z = U / sqrt(Vr)      p = erfc(sqrt(chi2 / 2.0))      beta = U / Vr      se = 1.0 / sqrt(Vr)
 *   p is the upper tail of chi-square with one degree of freedom.  beta and se are the ONE-STEP, score-based estimates of the log odds ratio
 *   per allele (the first Newton step from the null), not a Wald fit: they agree with it for small effects only.  All five are a quiet NaN
 *   where Vr is not > 0 or an input is NaN.  Each output pointer may be NULL; count == 0 is FMH_OK; a NULL input FMH_ERR_INVALID.
 * Not built: Wald and Firth estimates, the saddle-point correction for unbalanced case / control, per-phenotype missing values,
 *   sharding over devices (a caller splits rows), run_vcf wiring, u8 rows.  (The random effect of the relationship matrix is for
 *   quantitative phenotypes: the mixed-model scan below; a logistic mixed model is not built.)
 */
#define FMH_LOGISTIC_FITTED 0
#define FMH_LOGISTIC_ONE_CLASS 1      /* no case or no control */
#define FMH_LOGISTIC_NOT_CONVERGED 2  /* 25 Newton steps without max |delta| < 1e-8 */
#define FMH_LOGISTIC_PIVOT 3          /* a Cholesky pivot that is not > 0 */
#define FMH_LOGISTIC_ZERO_WEIGHT 4    /* some w_i = mu_i (1 - mu_i) is not > 0 */
#define FMH_LOGISTIC_BASIS_LOST 5     /* a column of the whitened design is collinear */
int fmh_assoc_homalt_sums(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */,
                          size_t n_samples, size_t row_begin, size_t row_count, const int32_t* h_values /* [n_samples][n_columns] */,
                          size_t n_columns, long long* d_homalt_sum /* [row_count][n_columns], device, written */, void* stream);
int fmh_logistic_null(const double* h_phenotypes /* [n][n_phenotypes], 0.0 or 1.0 */, const double* h_covariates_or_null /* [n][n_covariates] */,
                      size_t n, size_t n_phenotypes, size_t n_covariates, int32_t* h_values /* n * n_phenotypes * (n_covariates + 3) entries */,
                      int32_t* h_exponent, long long* h_total /* n_phenotypes * (n_covariates + 3) entries each */, uint8_t* h_fitted,
                      int32_t* h_reason, int32_t* h_iterations, uint64_t* h_n_cases /* [n_phenotypes] each */, size_t* h_n_basis,
                      uint8_t* h_dropped_or_null /* [n_covariates] */);   /* host only, no device */
int fmh_logistic_score(const long long* d_dosage_sum, const long long* d_called_sum /* [n_rows][n_phenotypes * (n_basis + 3)] each */,
                       const long long* d_homalt_sum /* [n_rows][n_phenotypes] */, const uint32_t* d_hom_ref, const uint32_t* d_het,
                       const uint32_t* d_hom_alt /* [n_rows] each */, size_t n_rows, const long long* h_total,
                       const int32_t* h_exponent /* [n_phenotypes * (n_basis + 3)] each, host */, size_t n_basis, size_t n_phenotypes,
                       double* d_score, double* d_variance /* [n_rows][n_phenotypes] each, device, written */, int device, void* stream);
int fmh_logistic_score_host(const long long* h_dosage_sum, const long long* h_called_sum, const long long* h_homalt_sum, const uint32_t* h_hom_ref,
                            const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_rows, const long long* h_total, const int32_t* h_exponent,
                            size_t n_basis, size_t n_phenotypes, double* h_score, double* h_variance);   /* host only, no device */
int fmh_logistic_stats(const double* h_score, const double* h_variance, size_t count, double* h_chi2, double* h_z, double* h_p, double* h_beta,
                       double* h_se /* [count] each, or NULL */);   /* host only, no device */

/* ---- polygenic scores: exact per-sample weighted dosage sums (an addition: the reference has none) ---------------------------------------
 * What a study does with the beta column of an association scan: for every sample the sum over sites of weight x dosage, for up to 64
 * weight columns at once (plink's --score; with centred weights the projection step of a genotype PCA).  It is fmh_assoc_sums transposed:
 * the contraction runs over ROWS and the result is per SAMPLE.  Matrix, samples, c_i(r) and g_i(r) are fmh_assoc_sums': ploidy 2, a packed
 * image, sample s owns columns 2s and 2s+1, the genotype is called iff both entries are called and both alleles are <= 1, every class is
 * masked with the called plane.  n = n_samples; i is a position in the sample list.
 *
 * Device sums (fmh_score_sums).  Given V[row_count][K] and optionally U[row_count][K] (i32, host, row-major by row of the range), for every
 * selected sample i, in list order, and k < K:
 *     S[i][k] = sum_r c_i(r) * g_i(r) * V[r][k]   (dosage sum)        C[i][k] = sum_r c_i(r) * U[r][k]   (called sum; optional)
 *   Both are exact `long long` device buffers [n][K], WRITTEN (not added).  Limits: 1 <= K <= 64, |V|, |U| <= 2^30, row_count <= 2^21, so
 *   |S| <= 2^52, |C| <= 2^51 and |S + (T_U - C)| < 2^53 (T_U the column totals of U): every sum converts to f64 without rounding.  V and U
 *   travel as four signed base-256 digits and the contraction over rows runs on the int8 matrix cores straight from the bit planes; an i32
 *   digit accumulator of one work item holds at most 2 * item_rows * 128 <= 2^30; the items' i64 partials are added in row-block order.
 *   C is computed iff BOTH h_called_values_or_null and d_called_sum_or_null are given.  A matrix that is biallelic with nothing missing
 *   runs no second contraction: C is filled with the column totals of U.  Enqueues on `stream` and synchronises it.
 *   Refusals, all before any launch, in this order.  FMH_ERR_INVALID: NULL matrix, dosage values or d_dosage_sum; called values without
 *   d_called_sum or the reverse; n_samples == 0; K outside 1..64; row_count > 2^21; a value beyond +-2^30; a sample index out of range, or a
 *   list that is not strictly ascending (n_samples beyond the matrix's samples without a list); a row range past the matrix.
 *   FMH_ERR_UNSUPPORTED, with a message: ploidy != 2; a matrix without a packed image (u8 rows only: call fmh_matrix_pack first); digits
 *   and slabs above FMH_SCORE_BUDGET_BYTES (the message names the option).  row_count == 0 writes zeros and is FMH_OK.
 *   Options: FMH_SCORE_ITEM_ROWS = the most rows of a work item (default 4 096; rounded up to a multiple of 64).  FMH_SCORE_BUDGET_BYTES =
 *   the device bytes the call's digits (4 bytes per row and column, whole steps of 64 rows and groups of 16 columns) and slabs (8 bytes per
 *   row block, sample of the covered groups of 256 and column), each twice when C is contracted, may take (default 1 GiB).  Neither changes
 *   a result, nor do FMH_GRID_PER_CU and FMH_GRID_BLOCKS.
 *
 * Host functions (no device).  The operation order is fixed so that a plain Python loop over ints and floats reproduces every bit (the
 * library is built with -ffp-contract=off).
 *   fmh_score_exponents: h_weights f64 [n_rows][K] -> e[K].  e_k = the largest integer with 2 * max_r |w_rk| * 2^e_k <= 2^30 - the rule of
 *     fmh_assoc_prepare's step 4 at 2 * max, taken without forming the product: max = f * 2^x with f in [0.5, 1) gives e = 30 - x when
 *     f == 0.5, else 29 - x; e_k = 0 for a column of zeros.  The headroom of 2 is for U below (mu <= 2).  The exponent depends on the weights
 *     alone, so a scan walked in row chunks uses one exponent and its i64 chunk sums add exactly.  Refusals (FMH_ERR_INVALID): K outside
 *     1..64, a NULL pointer (h_weights with n_rows == 0 excepted), a non-finite weight.
 *   fmh_score_values: the weights of a row chunk, e[K], and either the chunk's three u32 QC site tracks (fmh_genotype_counts, same rows and
 *     samples) or all three NULL -> V [n_rows][K], U [n_rows][K] with its exact i64 column totals T_U[K] (both or neither; they need the
 *     tracks), h_row_used u8 [n_rows].  Per row: N = hom_ref + het + hom_alt (without tracks every row counts as called).  A row with N == 0,
 *     or whose weights are all zero, is unused: h_row_used = 0 and its V and U rows are zero.  Otherwise
 *         mu = (double)(het + 2 * hom_alt) / (double)N;   V = (int32) rint(ldexp(w, e));   U = (int32) rint(ldexp(mu * w, e))
 *     with the product mu * w taken first, in f64.  Refusals (FMH_ERR_INVALID): K outside 1..64; NULL exponents; one or two tracks; U without
 *     T_U or the reverse, or without tracks; with n_rows > 0 a NULL weights, V or h_row_used; a non-finite weight; a weight with
 *     |w| * 2^e > 2^29 (the exponent is not this column's).
 *   fmh_score_stats: S, C, T_U, e, a mode -> f64 [n][K].  The integer in parentheses is formed in i64.
 *         FMH_SCORE_MEAN    ldexp((double)(S + (T_U - C)), -e)   missing genotypes mean-imputed (plink's default)
 *         FMH_SCORE_CENTER  ldexp((double)(S - C), -e)           sum of c (g - mu) w: missing contributes 0
 *         FMH_SCORE_ZERO    ldexp((double)S, -e)                 missing contributes 0; needs neither C nor T_U
 *     Sums of row chunks are added (i64) before this call: S, C and T_U are plain sums over rows.  Refusals (FMH_ERR_INVALID): K outside
 *     1..64; an unknown mode; with n_samples > 0 a NULL S, e or output, C where the mode needs it, T_U in mode mean.  n_samples == 0 is FMH_OK.
 * Not built: a run_vcf flag, sharding over devices (a caller splits rows and adds), haploid or u8-row matrices, variance-standardised
 *   weights (a caller divides), a genotype-PCA projection API (FMH_SCORE_CENTER is its kernel), per-sample score files.
 */
#define FMH_SCORE_MEAN 0
#define FMH_SCORE_CENTER 1
#define FMH_SCORE_ZERO 2
int fmh_score_sums(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                   size_t row_begin, size_t row_count, const int32_t* h_dosage_values /* [row_count][n_columns] */,
                   const int32_t* h_called_values_or_null /* [row_count][n_columns] */, size_t n_columns,
                   long long* d_dosage_sum /* [n_samples][n_columns], device, written */,
                   long long* d_called_sum_or_null /* [n_samples][n_columns], device, written */, void* stream);
int fmh_score_exponents(const double* h_weights /* [n_rows][n_columns] */, size_t n_rows, size_t n_columns,
                        int32_t* h_exponent /* [n_columns] */);   /* host only, no device */
int fmh_score_values(const double* h_weights /* [n_rows][n_columns] */, size_t n_rows, size_t n_columns, const int32_t* h_exponent /* [n_columns] */,
                     const uint32_t* h_hom_ref_or_null, const uint32_t* h_het_or_null, const uint32_t* h_hom_alt_or_null /* [n_rows] each, or all NULL */,
                     int32_t* h_dosage_values /* [n_rows][n_columns] */, int32_t* h_called_values_or_null /* [n_rows][n_columns] */,
                     long long* h_called_total_or_null /* [n_columns] */, uint8_t* h_row_used /* [n_rows] */);   /* host only, no device */
int fmh_score_stats(const long long* h_dosage_sum, const long long* h_called_sum_or_null /* [n_samples][n_columns] each */,
                    const long long* h_called_total_or_null, const int32_t* h_exponent /* [n_columns] each */, size_t n_samples, size_t n_columns,
                    int mode /* FMH_SCORE_* */, double* h_score /* [n_samples][n_columns] */);   /* host only, no device */

/* ---- runs of homozygosity: per-sample ROH scan from the bit planes (an addition: the reference has none) --------------------------------
 * Where along the rows each individual is autozygous and for how long: PLINK's --homozyg sliding window, every quantity an integer.  This
 * text is the DEFINITION; the device (fmh_roh_scan), the host twin (fmh_roh_scan_host) and a plain Python loop agree on every integer.
 * Matrix, samples, `called` and dosage are fmh_genotype_counts': ploidy 2, a packed image, sample s owns columns 2s and 2s+1, the genotype
 * is called iff both entries are called and both alleles are <= 1, every plane is masked with the called plane (row_gap / row_hi are
 * honoured).  n = n_samples; i is a position in the sample list.
 * Kept rows.  k = 0 .. K-1 are the rows of [row_begin, row_begin + row_count) whose h_keep_or_null byte is non-zero (NULL: every row), in
 *   ascending order.  x(k) is the position of kept row k: h_positions_or_null[variants] u32, indexed by matrix row as fmh_ehh_scan takes it
 *   and non-decreasing over the range; NULL means x is the row number.  Only differences of x are used.
 * State of sample i at kept row k: HOM (called, dosage 0 or 2), HET (called, dosage 1), MISS (not called).
 * Parameters (fmh_roh_params), all integers: window W (1..64), window_het, window_missing, need[65], min_sites, min_length, max_gap
 *   (0 = none), max_bp_per_site (0 = none), max_het, max_missing (UINT32_MAX = none), n_bins <= 8 with bin_edges[0 .. n_bins-2] strictly
 *   ascending (n_bins bins have n_bins - 1 edges; the other entries are ignored).
 * Windows.
 *   1. Window t, 0 <= t <= K-W, covers kept rows [t, t+W).  K < W: no window and no run.
 *   2. Window t is homozygous for a sample iff its HET count <= window_het and its MISS count <= window_missing.
 * In-run rows.
 *   3. Row k is covered by the windows t in [max(0, k-W+1), min(k, K-W)]: n_cov(k) of them (fewer near both ends), n_hom(k) of those
 *      homozygous.  Row k is IN A RUN iff n_hom(k) >= need[n_cov(k)].
 *   4. fmh_roh_need(threshold, W, need) (host only) fills need[c] for c = 1..W: the smallest integer h >= 1 with
 *      (double)h >= threshold * (double)c, the product formed once in f64; need[0] and need[W+1 ..] are set to 0 and never read.  This is
 *      PLINK's --homozyg-window-threshold made an integer table once: the device compares integers only.  Refusals (FMH_ERR_INVALID):
 *      NULL need, W outside 1..64, a threshold that is not within 0 .. 2 (above 1 no row can be in a run; need stays a byte).
 * Runs.
 *   5. break(k), k >= 1, iff max_gap > 0 and x(k) - x(k-1) > max_gap.
 *   6. A run [f, l] is a maximal stretch of consecutive kept rows that are all in a run, with no break(k) for f < k <= l.
 *   7. n_sites = l - f + 1; n_het and n_missing = its rows in state HET / MISS; length = x(l) - x(f) + 1 (u64).
 *   8. A run QUALIFIES iff n_sites >= min_sites, length >= min_length, n_het <= max_het, n_missing <= max_missing, and max_bp_per_site == 0
 *      or length <= max_bp_per_site * n_sites (the product in u64).
 * Outputs, exact integers.  Per selected sample, at its list position, device u64 [n], WRITTEN (fmh_roh_out; any pointer may be NULL):
 *   n_runs, sum_sites, sum_length, longest_length over the sample's qualifying runs, and with n_bins > 0 bin_runs[n][n_bins] and
 *   bin_length[n][n_bins]: a run falls in bin b = the number of edges <= its length.
 *   Segments (optional): fmh_roh_segment { sample, n_sites, n_het, n_missing, first_row, last_row }; `sample` is i, the run's position in
 *   the sample list; rows are those of the matrix relative to row_begin.  d_segments_or_null is a DEVICE buffer of segment_capacity
 *   elements (NULL: capacity 0); *h_segment_count receives the exact number of qualifying runs of the call even when it exceeds the
 *   capacity, and the buffer then holds min(count, capacity) distinct true segments in unspecified order.  fmh_roh_sort_segments (host
 *   only) orders host segments by (sample, first_row).
 * fmh_roh_scan enqueues on `stream` and synchronises it.  K == 0 or K < W is FMH_OK with zero tables and count 0.
 * Refusals, all before any launch, in this order.  FMH_ERR_INVALID: NULL matrix or params; n_samples == 0; a sample index out of range or
 *   a list that is not strictly ascending; a row range past the matrix; window outside 1..64; n_bins > 8 or edges not strictly ascending;
 *   positions that descend in the range; every output NULL (no table, no segment buffer, no count); a segment buffer without a count
 *   pointer.  FMH_ERR_UNSUPPORTED, with a message: ploidy != 2; a matrix without a packed image (call fmh_matrix_pack first); a range of
 *   2^32 - 1 rows or more.
 * Option: FMH_ROH_ITEM_ROWS = the most kept rows of a work item (default 4 096; rounded up to a multiple of 64).  It changes no result, nor
 *   do FMH_GRID_PER_CU and FMH_GRID_BLOCKS.
 * fmh_roh_scan_host (host only, no device): the same parameters over h_state u8 [K][n] (0 HOM, 1 HET, 2 MISS) and h_x u32 [K]
 *   (non-decreasing; NULL = k); the tables and segments are host arrays (fmh_roh_out's pointers are then host pointers), rows of a
 *   segment are kept rows k.  A serial state machine over the whole range.  Refusals (FMH_ERR_INVALID): NULL params; n == 0; NULL state
 *   with K > 0; window, bins, descending x, outputs and segments as above; a state above 2.
 * Not built: sharding over devices, run_vcf wiring, u8 rows, end-trimming of hets at run edges (PLINK trims; a run here is the maximal
 *   stretch of in-run rows).
 */
typedef struct {
  uint32_t window, window_het, window_missing;
  uint8_t need[65];                 /* need[c], c = 1..window (fmh_roh_need) */
  uint8_t reserved[3];
  uint32_t min_sites, min_length, max_gap, max_bp_per_site, max_het, max_missing;
  uint32_t n_bins;                  /* 0..8 */
  uint32_t bin_edges[7];            /* the first n_bins - 1 are read */
} fmh_roh_params;
typedef struct { uint32_t sample, n_sites, n_het, n_missing; uint64_t first_row, last_row; } fmh_roh_segment;
typedef struct {
  unsigned long long *d_n_runs, *d_sum_sites, *d_sum_length, *d_longest_length;  /* each [n], written; any may be NULL */
  unsigned long long *d_bin_runs, *d_bin_length;                                  /* each [n][n_bins], written; any may be NULL */
} fmh_roh_out;
int fmh_roh_scan(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                 size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count] */,
                 const uint32_t* h_positions_or_null /* [variants] */, const fmh_roh_params* params, const fmh_roh_out* out_or_null,
                 fmh_roh_segment* d_segments_or_null, size_t segment_capacity, uint64_t* h_segment_count /* may be NULL without a buffer */,
                 void* stream);
int fmh_roh_scan_host(const uint8_t* h_state /* [n_kept][n_samples] */, const uint32_t* h_x_or_null /* [n_kept] */, size_t n_kept, size_t n_samples,
                      const fmh_roh_params* params, const fmh_roh_out* out_or_null /* host pointers */, fmh_roh_segment* h_segments_or_null,
                      size_t segment_capacity, uint64_t* h_segment_count);   /* host only, no device */
int fmh_roh_need(double threshold, uint32_t window, uint8_t* need /* [65] */);   /* host only, no device */
int fmh_roh_sort_segments(fmh_roh_segment* h_segments, size_t count);   /* host only, no device */

/* ---- IBD segments: pairwise shared-segment scan from the bit planes (an addition: the reference has none) -------------------------------
 * Where along the rows two diploid samples share a segment identical by descent and for how long: the IBS detector of IBIS, TRUFFLE,
 * GERMLINE and PLINK's --segment on unphased genotypes, every quantity an integer.  This text is the DEFINITION; the device
 * (fmh_ibd_scan), the host twin (fmh_ibd_scan_host) and a plain Python loop agree on every integer.
 * Matrix, samples, `called` and dosage are fmh_genotype_counts' / fmh_roh_scan's: ploidy 2, a packed image, sample s owns columns 2s and
 * 2s+1, the genotype is called iff both entries are called and both alleles are <= 1, every plane is masked with the called plane
 * (row_gap / row_hi are honoured).  n = n_samples; i < j are positions in the sample list; the pairs are all n (n - 1) / 2 unordered
 * pairs of the list.
 * Kept rows k = 0 .. K-1, their positions x(k) and break(k) are exactly fmh_roh_scan's ("Kept rows" and rule 5): the h_keep_or_null
 *   bytes; h_positions_or_null[variants] u32 indexed by matrix row, non-decreasing over the range, NULL meaning the row number;
 *   break(k), k >= 1, iff max_gap > 0 and x(k) - x(k-1) > max_gap.
 * State of pair (i, j) at kept row k: MISS if either genotype is not called; otherwise DISC iff
 *   mode FMH_IBD1: one dosage is 0 and the other is 2 (opposite homozygotes, IBS0);
 *   mode FMH_IBD2: the dosages differ;
 *   otherwise CONC.
 * Runs.
 *   1. A run [f, l] is a maximal stretch of consecutive kept rows none of which is DISC, with no break(k) for f < k <= l.  MISS rows are
 *      compatible and may stand at either end: there is no trimming.  No error tolerance: a single DISC row ends a run.
 *   2. n_sites = l - f + 1; n_missing = the run's MISS rows; length = x(l) - x(f) + 1 (u64).
 *   3. A run QUALIFIES iff n_sites >= min_sites, length >= min_length, n_missing <= max_missing (UINT32_MAX = none), and
 *      max_bp_per_site == 0 or length <= max_bp_per_site * n_sites (the product in u64).
 * Parameters: fmh_ibd_params { mode, min_sites, min_length, max_gap (0 = none), max_bp_per_site (0 = none), max_missing }.
 * Outputs, exact integers.  Tables (fmh_ibd_out; any pointer may be NULL), each a device u64 [n][n], WRITTEN, not added into: both
 *   triangles are filled and the diagonal is 0; over the pair's qualifying runs n_segments, sum_sites, sum_length, longest_length.
 *   Segments (optional): fmh_ibd_segment { a, b, n_sites, n_missing, first_row, last_row }; a < b are list positions; rows are those of
 *   the matrix relative to row_begin.  d_segments_or_null is a DEVICE buffer of segment_capacity elements (NULL: capacity 0);
 *   *h_segment_count receives the exact number of qualifying runs of the call even when it exceeds the capacity, and the buffer then
 *   holds min(count, capacity) distinct true segments in unspecified order.  fmh_ibd_sort_segments (host only) orders host segments by
 *   (a, b, first_row).
 * fmh_ibd_scan enqueues on `stream` and synchronises it.  K == 0 or n == 1 is FMH_OK with zero tables and count 0.
 * Refusals, all before any launch, in this order.  FMH_ERR_INVALID: NULL matrix or params; n_samples == 0; a sample index out of range or
 *   a list that is not strictly ascending; a row range past the matrix; a mode other than FMH_IBD1 / FMH_IBD2; positions that descend in
 *   the range; every output NULL (no table, no segment buffer, no count); a segment buffer without a count pointer.
 *   FMH_ERR_UNSUPPORTED, with a message: ploidy != 2; a matrix without a packed image (call fmh_matrix_pack first); a range of 2^32 - 1
 *   rows or more; scratch (the sample-major bit image plus the block records) above FMH_IBD_BUDGET_BYTES (the message names the bytes
 *   needed and the option); more than 2^31 work items.
 * Options: FMH_IBD_ITEM_ROWS = the kept rows of a row block (rounded up to a multiple of 64; default: one block when the pair tiles alone
 *   give every workgroup of the grid several items, otherwise as many equal blocks as reach that, fewer when the budget asks);
 *   FMH_IBD_BUDGET_BYTES (default 4 GiB) bounds the scratch of a call.  Neither changes a result, nor do FMH_GRID_PER_CU and
 *   FMH_GRID_BLOCKS.
 * fmh_ibd_scan_host (host only, no device): the same parameters over h_dosage u8 [K][n] (0, 1, 2; 3 = not called) and h_x u32 [K]
 *   (non-decreasing; NULL = k); the tables and segments are host arrays (fmh_ibd_out's pointers are then host pointers), rows of a
 *   segment are kept rows k.  A serial loop per pair over the whole range.  Refusals (FMH_ERR_INVALID): NULL params; n == 0; NULL dosage
 *   with K > 0; mode, descending x, outputs and segments as above; a dosage above 3.  FMH_ERR_UNSUPPORTED: 2^32 - 1 kept rows or more.
 * Not built: error tolerance inside a segment, trimming MISS rows at run ends, a minimum count of informative sites, explicit pair lists
 *   or pairs between two sample lists, genetic-map lengths, length bins on the device, sharding over devices, run_vcf wiring, u8 rows.
 */
#define FMH_IBD1 1
#define FMH_IBD2 2
typedef struct { uint32_t mode, min_sites, min_length, max_gap, max_bp_per_site, max_missing; } fmh_ibd_params;
typedef struct { uint32_t a, b, n_sites, n_missing; uint64_t first_row, last_row; } fmh_ibd_segment;
typedef struct {
  unsigned long long *d_n_segments, *d_sum_sites, *d_sum_length, *d_longest_length;  /* each [n][n], written; any may be NULL */
} fmh_ibd_out;
int fmh_ibd_scan(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                 size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count] */,
                 const uint32_t* h_positions_or_null /* [variants] */, const fmh_ibd_params* params, const fmh_ibd_out* out_or_null,
                 fmh_ibd_segment* d_segments_or_null, size_t segment_capacity, uint64_t* h_segment_count /* may be NULL without a buffer */,
                 void* stream);
int fmh_ibd_scan_host(const uint8_t* h_dosage /* [n_kept][n_samples]: 0, 1, 2, 3 = not called */, const uint32_t* h_x_or_null /* [n_kept] */,
                      size_t n_kept, size_t n_samples, const fmh_ibd_params* params, const fmh_ibd_out* out_or_null /* host pointers */,
                      fmh_ibd_segment* h_segments_or_null, size_t segment_capacity, uint64_t* h_segment_count);   /* host only, no device */
int fmh_ibd_sort_segments(fmh_ibd_segment* h_segments, size_t count);   /* host only, no device */

/* ---- LD clumping: genotype r^2 around index sites (an addition: the reference has none) ---------------------------------------------
 * The step between an association scan and a polygenic score (PLINK --clump): sites are taken in order of ascending p; each one not yet
 * claimed becomes an index site and claims every nearby site whose genotype r^2 with it reaches a threshold.  THE definition: the device
 * (fmh_clump, fmh_geno_ld_pairs), the host twins and a plain Python loop agree on every integer and every bit of r^2.
 * Matrix, samples, called, dosage: fmh_genotype_counts' / fmh_roh_scan's.  Ploidy 2, a packed image; sample s owns columns 2s and 2s + 1;
 *   a genotype is called iff both entries are called and both alleles are <= 1; every plane is masked with the called plane (junk bits
 *   under uncalled entries are legal); row_gap / row_hi are honoured.  n = n_samples; the dosage is g in {0, 1, 2}.
 * Genotype LD of two rows a, b over the selected samples (fmh_geno_ld_counts, eight u32, the last two reserved and written 0):
 *   n = samples called at both rows; sum_a = sum g_a, sum_b, sq_a = sum g_a^2, sq_b, cross = sum g_a g_b, each over those n samples.
 *   In int64: cov = n cross - sum_a sum_b, va = n sq_a - sum_a^2, vb likewise.
 *   r2 = ((double)cov * (double)cov) / ((double)va * (double)vb), built with -ffp-contract=off.  va == 0 || vb == 0 (this includes
 *   n == 0) gives a quiet NaN.  The squared Pearson correlation of the two dosage vectors over the jointly called samples (PLINK --r2's
 *   default statistic); every integer stays below 2^53 for rows of at most 600 000 columns.  a == b is allowed and gives 1.0 or NaN.
 *   From the bit planes, with A the alt-allele bits of a row masked to its called genotypes and swap() exchanging the two bits of every
 *   sample: cross = popc(A_a & A_b) + popc(swap(A_a) & A_b), sum g^2 = popc(A) + 2 popc(hom-alt).
 * Clumping, parameters fmh_clump_params { p1, p2, r2, window }:
 *   1. Kept rows and positions x are fmh_roh_scan's: the h_keep_or_null bytes; h_positions_or_null [variants] u32, indexed by matrix row
 *      and non-decreasing over the range; NULL = x is the row number.
 *   2. h_p is f64 [row_count].  A row is a PARTICIPANT iff it is kept, its p is not NaN and p <= p2; a participant is a CANDIDATE iff
 *      p <= p1.
 *   3. Candidates are visited by ascending (p, row), compared as f64.  A candidate that is already claimed is skipped.  Otherwise it
 *      becomes an INDEX and owns itself; it then claims every participant j != i that is not yet owned (neither an index nor a member)
 *      with |x(j) - x(i)| <= window and r2(i, j) >= r2.  NaN never qualifies.
 *   4. A participant that no index claims stays unassigned.  There is no overlap option: a site belongs to the first index that reaches it.
 * Outputs are host arrays (rule 3 runs on the host, as fmh_ld_prune's does): h_index_of u32 [row_count]: the index's row relative to
 *   row_begin (an index names itself), UINT32_MAX for a row in no clump; h_r2_or_null f64 [row_count]: r2 of the row with its index by the
 *   formula above (an index with itself), NaN where index_of is UINT32_MAX; *h_n_clumps_or_null: the number of clumps.
 * fmh_clump enqueues on `stream` and synchronises it.  With no participant or no candidate it is FMH_OK with UINT32_MAX / NaN / 0 and no
 *   launch.  fmh_geno_ld_pairs gives the counts of P arbitrary row pairs (matrix rows) into a device array; fmh_clump calls it once at the
 *   end for the (index, member) pairs behind h_r2.
 * Refused before any launch, in this order.  FMH_ERR_INVALID: a NULL matrix, params, h_p or h_index_of; n_samples == 0; a bad sample
 *   list; a row range past the matrix; params that are NaN or do not satisfy 0 <= p1 <= p2 <= 1 and 0 <= r2 <= 1; a p of a kept row that
 *   is neither NaN nor within [0, 1]; positions that descend in the range.  For the pairs call also: a NULL list or output with P > 0; a
 *   row outside the matrix.  FMH_ERR_UNSUPPORTED, each with a message: ploidy != 2; no packed image; a range of 2^32 - 1 rows or more;
 *   threshold words above the budgets (FMH_CLUMP_HOST_BYTES for all candidates' bit rows on the host, FMH_CLUMP_BUDGET_BYTES when one tile
 *   row of candidates alone exceeds a launch's scratch; the message names the bytes needed and the option); more than 2^31 work items.
 * Host only, no device: fmh_geno_ld_r2 (the formula alone, P count records), fmh_geno_ld_pairs_host (counts of P row pairs of h_dosage u8
 *   [K][n]: 0, 1, 2; 3 = not called) and fmh_clump_host (the same rule over h_dosage, h_x u32 [K] or NULL = k, h_p f64 [K]; every given
 *   row counts as kept and rows are 0 .. K - 1).
 * Options (neither changes a result): FMH_CLUMP_BUDGET_BYTES (default 1 GiB), FMH_CLUMP_HOST_BYTES (default 8 GiB).
 */
typedef struct { uint32_t n, sum_a, sum_b, sq_a, sq_b, cross, reserved[2]; } fmh_geno_ld_counts;
typedef struct { double p1, p2, r2; uint32_t window; uint32_t reserved; } fmh_clump_params;
int fmh_clump(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
              size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count] */,
              const uint32_t* h_positions_or_null /* [variants] */, const double* h_p /* [row_count] */, const fmh_clump_params* params,
              uint32_t* h_index_of /* [row_count] */, double* h_r2_or_null /* [row_count] */, uint64_t* h_n_clumps_or_null, void* stream);
int fmh_geno_ld_pairs(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, const uint32_t* h_rows_a /* [P], matrix rows */,
                      const uint32_t* h_rows_b /* [P] */, size_t P, fmh_geno_ld_counts* d_counts /* [P], device, written */, void* stream);
int fmh_geno_ld_r2(const fmh_geno_ld_counts* h_counts, size_t P, double* h_r2);   /* host only, no device */
int fmh_geno_ld_pairs_host(const uint8_t* h_dosage /* [K][n]: 0, 1, 2, 3 = not called */, size_t K, size_t n, const uint32_t* h_rows_a,
                           const uint32_t* h_rows_b, size_t P, fmh_geno_ld_counts* h_counts);   /* host only, no device */
int fmh_clump_host(const uint8_t* h_dosage /* [K][n] */, const uint32_t* h_x_or_null /* [K] */, const double* h_p /* [K] */, size_t K, size_t n,
                   const fmh_clump_params* params, uint32_t* h_index_of /* [K] */, double* h_r2_or_null /* [K] */,
                   uint64_t* h_n_clumps_or_null);   /* host only, no device */

/* ---- LD scores and LD score regression (an addition: the reference has none) -----------------------------------------------------------
 * What a study computes from an association scan's chi^2 column: the LD score of every site, l_i = the sum of genotype r^2 over the sites
 * within a window of site i (ldsc --l2, GCTA --ld-score), and the regression of chi^2 on it, whose intercept separates confounding from
 * polygenicity and whose slope is the SNP heritability.  THE definition: the device (fmh_ld_scores), the host twin (fmh_ld_scores_host)
 * and a plain Python loop agree on every integer.
 * Matrix, samples, called, dosage, kept rows and positions are fmh_clump's (rule 1 there): ploidy 2, a packed image, every plane masked
 *   with the called plane, row_gap / row_hi honoured; h_keep_or_null; h_positions_or_null u32 [variants], non-decreasing over the range,
 *   NULL = x is the row number.  Parameters fmh_ldscore_params { window, flags }; flags is 0 or FMH_LDSCORE_ADJUST.
 * Pair term of two kept rows i, j (j = i included): the six integers are fmh_geno_ld_counts over the selected samples and r2 is the
 *   fmh_geno_ld_r2 formula, bit for bit.  The pair is SKIPPED when r2 is NaN and, with FMH_LDSCORE_ADJUST, also when the joint called
 *   count n < 3.  Otherwise t = r2 without FMH_LDSCORE_ADJUST and t = r2 - (1.0 - r2) / (double)(n - 2) with it (ldsc's bias correction,
 *   in that operation order, built with -ffp-contract=off), and q = llrint(ldexp(t, 40)), round half to even.
 * Per kept row i: partners[i] = the number of kept rows j with |x_j - x_i| <= window (i itself is one), counted[i] = the number of those
 *   that are not skipped, Q[i] = the sum of q over them as int64.  Rows that are not kept get 0, 0, 0.  The sum of integers is the same in
 *   every order, so tiles, the symmetry r2_ij = r2_ji and atomic adds change nothing; the quantisation is at most 2^-41 per term.
 *   fmh_ld_score_values: score = (double)Q * 2^-40, NaN where counted == 0.
 * fmh_ld_scores: host outputs h_q i64 [row_count], h_partners_or_null u32 [row_count], h_counted u32 [row_count], every entry written;
 *   it enqueues on `stream` and synchronises it.  No kept row is FMH_OK with zeros and no launch.
 * Refused before any launch, in this order.  FMH_ERR_INVALID: a NULL matrix, params, h_q or h_counted; n_samples == 0; a bad sample list; a
 *   row range past the matrix; flags other than 0 or FMH_LDSCORE_ADJUST; positions that descend in the range.  FMH_ERR_UNSUPPORTED, each
 *   with a message: ploidy != 2; no packed image (the message names fmh_matrix_pack); a range of 2^32 - 1 rows or more; a row with more than
 *   2^22 partners (so that |Q| < 2^63); more than 2^31 work items; a launch's scratch above FMH_LDSCORE_BUDGET_BYTES (default 1 GiB): the
 *   scratch is 28 bytes per kept row plus 8 bytes per work item (a pair of 64-row tiles of kept rows that holds a partner pair); the items
 *   are walked in chunks under the budget, and a budget below 28 bytes per kept row plus one item is refused with the bytes needed.  The
 *   option changes no result.
 * Host only, no device: fmh_ld_scores_host (the same rule over h_dosage u8 [K][n]: 0, 1, 2; 3 = not called, h_x u32 [K] or NULL = k; every
 *   given row counts as kept; refusals as fmh_clump_host's), fmh_ld_score_values and fmh_ldsc_regress.
 * LD score regression, fmh_ldsc_regress(chi2 [K], score [K], w_score_or_null [K] (NULL = score), K, N, M, blocks, fixed_intercept_or_null):
 *   a site is USED iff its chi2, score and w_score are finite; U used sites, in ascending order, B = min(blocks, U) blocks
 *   [floor(bU/B), floor((b+1)U/B)).  x = N * l / M; the model is E[chi2] = a + h x.  Start a = 1.0 (or the fixed intercept) and
 *   h = M * (mean chi2 - 1.0) / (N * mean l).  Weights of an estimate (a, h), hc = h clipped to [0, 1]:
 *   c = a + ((hc * N) * max(l, 1.0)) / M,  w = 1.0 / (max(lw, 1.0) * (2.0 * (c * c))).
 *   Three weighted least-squares fits, each with the weights of the previous estimate.  Sums in ascending site order:
 *   Sw = sum w, Sx = sum w x, Sxx = sum (w x) x, Sy = sum w y, Sxy = sum (w x) y; det = Sw Sxx - Sx Sx, h = (Sw Sxy - Sx Sy) / det,
 *   a = (Sxx Sy - Sx Sxy) / det; with a fixed intercept h = (Sxy - a Sx) / Sxx.  Standard errors: delete-one-block jackknife of the last
 *   fit with its weights held; per-block sums, the sums without block b added in ascending block order, pseudo-values
 *   (double)B * theta - (double)(B - 1) * theta_(-b), se = sqrt(var(pseudo, ddof 1) / B).  ratio = (a - 1) / (mean chi2 - 1);
 *   lambda_gc = median chi2 / 0.4549364231195724 (an even U takes (lo + hi) / 2.0).  intercept_se is NaN with a fixed intercept.
 *   Built with -ffp-contract=off: a plain loop over doubles reproduces every bit.
 *   Refused (FMH_ERR_INVALID) before any arithmetic: a NULL chi2, score or out; N or M not finite or <= 0; a fixed intercept that is not
 *   finite; blocks < 2; fewer than 2 used sites per fitted parameter and block (U < 2 P B, P = 2, or 1 with a fixed intercept); a
 *   negative chi2 among the used sites.
 */
#define FMH_LDSCORE_ADJUST 1u
typedef struct { uint32_t window; uint32_t flags; } fmh_ldscore_params;
typedef struct { double h2, h2_se, intercept, intercept_se, ratio, mean_chi2, lambda_gc; uint64_t n_used, blocks; } fmh_ldsc_out;
int fmh_ld_scores(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                  size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count] */,
                  const uint32_t* h_positions_or_null /* [variants] */, const fmh_ldscore_params* params, int64_t* h_q /* [row_count] */,
                  uint32_t* h_partners_or_null /* [row_count] */, uint32_t* h_counted /* [row_count] */, void* stream);
int fmh_ld_scores_host(const uint8_t* h_dosage /* [K][n]: 0, 1, 2, 3 = not called */, const uint32_t* h_x_or_null /* [K] */, size_t K, size_t n,
                       const fmh_ldscore_params* params, int64_t* h_q /* [K] */, uint32_t* h_partners_or_null /* [K] */,
                       uint32_t* h_counted /* [K] */);   /* host only, no device */
int fmh_ld_score_values(const int64_t* h_q, const uint32_t* h_counted, size_t K, double* h_score);   /* host only, no device */
int fmh_ldsc_regress(const double* h_chi2, const double* h_score, const double* h_w_score_or_null, size_t K, double N, double M, uint64_t blocks,
                     const double* fixed_intercept_or_null, fmh_ldsc_out* out);   /* host only, no device */

/* ---- genomic relationship matrix and genotype PCA (an addition: the reference's PCA is the haplotype PCA above) ---------------------------
 * The per-sample link of the cohort chain QC -> fmh_ld_prune -> fmh_kinship_counts -> PCA -> association: the matrix GCTA --make-grm and
 * PLINK --make-rel compute, and its top eigenvectors (PLINK --pca), the covariates of the association scans.
 * Matrix, samples, `called` and dosage are fmh_genotype_counts': ploidy 2, a packed image, sample s owns columns 2s and 2s + 1; the genotype
 * of s at row r is called iff both entries are called and both alleles are <= 1 (classes hom-ref, het, hom-alt, not called); the dosage is
 * g in {0, 1, 2}.  Sample lists, row ranges and keep masks are fmh_kinship_counts', under the same rules.
 *
 * Over the kept rows k (in ascending row order) and the selected samples:
 *   c_k = the number of called genotypes, a_k = the sum of their dosages (exact u32);  p_k = (double)a_k / (double)(2 * c_k), NaN where c_k = 0.
 *   A kept row is USABLE iff c_k >= 1 and 0 < a_k < 2 c_k.  A row that is not usable contributes nothing; it is reported, never refused.
 *   MAF and call-rate filters are the caller's (the keep mask).
 *   Values of a usable row, the operation order fixed (the library is built with -ffp-contract=off; numpy reproduces the bits):
 *     mean = 2.0 * p;  var = mean * (1.0 - p);  z(g) = (double)g - mean for g = 0, 1, 2
 *     FMH_GRM_STANDARDIZED (GCTA, PLINK): z(g) = ((double)g - mean) / sqrt(var)
 *     FMH_GRM_CENTERED (VanRaden 1): z(g) as above;  scale = the sum of var over the usable rows, ascending, from 0.0
 *   A genotype that is not called has z = 0 (mean imputation), in both methods; a row that is not usable has z = (0, 0, 0).
 *   S[i][j] = sum over the usable rows of z_k(g_ik) z_k(g_jk): with mean imputation this is GCTA's sum over the rows called in both.
 *   N[i][j] = the number of usable rows called in both samples (u64).
 *   A = S / (double)m_usable (standardized) or S / scale (centered) with denominator FMH_GRM_SITES; S[i][j] / (double)N[i][j], NaN where
 *   N[i][j] = 0, with FMH_GRM_PAIRS (GCTA's), which takes FMH_GRM_STANDARDIZED only.  diag(A) - 1 is the per-sample inbreeding estimate.
 *
 * fmh_grm: out->d_products (f64 [n][n], device) is ADDED into - chromosomes held as separate matrices accumulate, as in kinship; the caller
 *   zeroes it first and adds up *h_usable_rows and *h_scale, which are WRITTEN with this call's.  Both triangles are filled; what one call adds
 *   is symmetric bit for bit and two runs give the same bits.  out->d_pair_sites (u64 [n][n], device, may be NULL; required with FMH_GRM_PAIRS)
 *   is ADDED into: it is fmh_kinship_counts' `both` over the usable rows.  out->h_called, h_allele_count (u32) and h_usable (u8) are host arrays
 *   of row_count entries (each may be NULL) whose first *h_kept_rows entries are written: c, a and the usable flag of the kept rows in row
 *   order; they come from fmh_genotype_counts' site tracks.  No kept row or no usable row: FMH_OK, nothing is added.
 *   How: the usable rows' 2-bit genotype codes go into a sample-major bit image (two planes, one u64 per 64 rows and sample), and S is a
 *   Gram on v_mfma_f64_16x16x4_f64 whose operand is {z(0), z(1), z(2), 0}[code]; K is split over workgroups while there are few tiles
 *   (FMH_GRM_SPLITS forces a count; 1 = none, 0 = by the tile count) and the partial tiles are added in split order.  Device memory from the
 *   pool: n^2 * 8 (the call's products) + the image (2 planes * 8 bytes per 64 rows and padded sample) + 32 bytes per row + 128 KiB per
 *   (tile, split) when K is split + 4 n^2 * 8 with d_pair_sites; the sum must stay within FMH_PCA_BUDGET_BYTES.  Neither option changes a
 *   result beyond the order of the sum.  Enqueues on `stream` and synchronises it.
 *   Refusals, all before any launch, in this order.  FMH_ERR_INVALID: NULL matrix; NULL params or out; d_products NULL; a method or
 *   denominator that is not listed, or FMH_GRM_PAIRS with FMH_GRM_CENTERED or without d_pair_sites; n_samples == 0.  FMH_ERR_UNSUPPORTED:
 *   ploidy != 2.  FMH_ERR_INVALID: a sample out of range or the list not strictly ascending; a row range past the matrix.
 *   FMH_ERR_UNSUPPORTED, with a message: a matrix without a packed image (u8 rows only: call fmh_matrix_pack first); 2^32 - 1 rows or more
 *   in the range, more than 2^24 samples; over budget.
 * Host only (no device), bit for bit what the definition says:
 *   fmh_grm_values: c, a of `rows` rows -> usable flags, p, z [rows][3], *scale, *n_usable (each output may be NULL).
 *   fmh_grm_finish: S, N (NULL unless FMH_GRM_PAIRS), m_usable, scale -> A.
 *   fmh_grm_host: the twin for CPU tests.  S [n][n] WRITTEN from a dosage table [K][n] (0, 1, 2; above 2 = not called): the counts, the
 *     values, then every entry summed over ascending k in plain f64; N, *n_usable and *scale as well (each may be NULL).
 * fmh_grm_eigen: the top n_components eigenpairs of the symmetric d_matrix [n][n] (device, OVERWRITTEN) through the solver of
 *   fmh_pca_eigen_scores (FMH_PCA_EIGEN): h_eigenvalues descending, h_eigenvectors [n][n_components], column k the unit eigenvector of
 *   h_eigenvalues[k], its component of the largest magnitude positive (on a tie the one of the lowest index).  FMH_ERR_INVALID: NULL argument,
 *   n == 0, n_components outside 1..n; FMH_ERR_UNSUPPORTED: n > 46 340.
 * Not built: sharding over devices (S is a plain sum over rows), run_vcf wiring, GCTA .grm.bin writers, dominance matrices, leave-one-
 *   chromosome-out sets, u8 rows.
 */
#define FMH_GRM_STANDARDIZED 0
#define FMH_GRM_CENTERED 1
#define FMH_GRM_SITES 0
#define FMH_GRM_PAIRS 1
typedef struct { uint32_t method, denominator; } fmh_grm_params;
typedef struct {
  double* d_products;                 /* [n][n], device, ADDED into */
  unsigned long long* d_pair_sites;   /* [n][n], device, ADDED into; may be NULL unless FMH_GRM_PAIRS */
  uint32_t *h_called, *h_allele_count; /* [row_count] host, the first *h_kept_rows written; may be NULL */
  uint8_t* h_usable;                  /* likewise */
  uint64_t* h_usable_rows;            /* written; may be NULL */
  double* h_scale;                    /* written; may be NULL */
} fmh_grm_out;
int fmh_grm(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
            size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count], as fmh_ld_prune writes it */,
            const fmh_grm_params* params, const fmh_grm_out* out, uint64_t* h_kept_rows /* may be NULL */, void* stream);
int fmh_grm_values(const uint32_t* h_called, const uint32_t* h_allele_count, size_t rows, uint32_t method, uint8_t* h_usable, double* h_p,
                   double* h_z /* [rows][3] */, double* h_scale, uint64_t* h_n_usable);   /* host only, no device */
int fmh_grm_finish(const double* h_products, const uint64_t* h_pair_sites_or_null, size_t n, const fmh_grm_params* params, uint64_t n_usable,
                   double scale, double* h_matrix);   /* host only, no device */
int fmh_grm_host(const uint8_t* h_dosage /* [K][n] */, size_t K, size_t n, uint32_t method, double* h_products, uint64_t* h_pair_sites_or_null,
                 uint64_t* h_n_usable, double* h_scale);   /* host only, no device */
int fmh_grm_eigen(int device, double* d_matrix, size_t n, size_t n_components, double* h_eigenvalues, double* h_eigenvectors);

/* ---- mixed-model association scan (an addition: the reference has none) ----------------------------------------------------------------------
 * The last link of the cohort chain: the single-variant test with the random effect of the relationship matrix A (EMMAX, GCTA --mlma,
 * FaST-LMM), exact in the eigenbasis of A.  With A = U diag(lambda) U^T and V = A + delta I, the per-site term g^T V^-1 g is a weighted sum of
 * squares of the rotated dosages U^T g: a K x n by n x rows product, which fmh_lmm_projections contracts on the f64 matrix cores straight from
 * the bit planes, with the weights and the coefficient rows the statistics need.
 * Matrix, samples, c_i(r), g_i(r), row ranges and row tables are fmh_assoc_sums'.  n = the number of selected samples, i = a position in the
 * sample list, u = 2^-53.  The library is built with -ffp-contract=off.
 *
 * fmh_lmm_projections (device).  d_basis f64 [n][K], device, row-major by sample position, 1 <= K <= 32 768 (it need not be square or
 *   orthogonal); d_weights f64 [P][K], 1 <= P <= 16; d_linear f64 [L][K], 1 <= L <= 64; outputs d_quad f64 [row_count][P] and d_lin f64
 *   [row_count][L]; optional host tracks h_called, h_allele_count (u32 [row_count]).  Per row r: c = the number of called genotypes, a = the
 *   number of alternate alleles among them - fmh_genotype_counts' site tracks, called from inside as fmh_grm does;
 *   mu = (double)a / (double)c, computed ON THE HOST and uploaded at 8 bytes per row (0 when c = 0); x_i(r) = g_i(r) where the genotype is
 *   called, else mu.
 *     T[r][k]    = sum_i  basis[i][k] * x_i(r)
 *     quad[r][p] = sum_k  weights[p][k] * T[r][k]^2
 *     lin[r][j]  = sum_k  linear[j][k]  * T[r][k]
 *   Both outputs are WRITTEN, every entry by one writer: nothing is zeroed, nothing is atomic.  The order of every sum is fixed by the kernel
 *   alone and two runs give the same bits; FMH_LMM_ITEM_ROWS (the most rows of a work item; default 4 096, or fewer whole passes of 128 rows
 *   where that many would leave compute units without an item), FMH_GRID_PER_CU and FMH_GRID_BLOCKS change no bit.  T is never stored.  Any
 *   order of the sums keeps |T^ - T| <= E_k = (n + 2) u sum_i |basis[i][k] x_i|, |lin^ - lin| <= sum_k |linear[j][k]| E_k + (K + 2) u sum_k
 *   |linear[j][k] T_k| and |quad^ - quad| <= sum_k |weights[p][k]| (2 |T_k| E_k + E_k^2) + (K + 3) u sum_k |weights[p][k]| T_k^2.
 *   Device memory from the pool: the basis as a padded image indexed by MATRIX sample number (64-sample x 64-component stages, zero rows for
 *   samples that are not selected), the coefficient image, 8 bytes per row and the tracks; the sum must stay within FMH_PCA_BUDGET_BYTES.
 *   Enqueues on `stream` and synchronises it.
 *   Refusals, all before any launch, in this order.  FMH_ERR_INVALID: a NULL matrix, input or output; n_samples == 0; a sample out of range
 *   or the list not strictly ascending; a row range past the matrix; K, P or L outside their limits.  FMH_ERR_UNSUPPORTED, each with a
 *   message: ploidy != 2; a matrix without a packed image; over budget.  row_count == 0 is FMH_OK.
 * fmh_lmm_projections_host: the twin for CPU tests.  h_dosage u8 [rows][n] (0, 1, 2; above 2 = not called); the same three formulas, every
 *   sum over ascending index in plain f64, the product with the weights as weights * (T * T).
 *
 * fmh_lmm_null (host only).  Eigenvalues lambda [n] (each taken as max(lambda_k, 0)), eigenvectors U [n][n] (column k belongs to
 *   lambda_k), phenotypes [n][P], covariates [n][c_in].  The design matrix is X = [1/sqrt(n) 1, Q]: Q = fmh_assoc_prepare's centred,
 *   twice-orthonormalised covariate basis with its drop rule and its `dropped` flags; q = c + 1 columns (*h_q).  Rotation X~ = U^T X,
 *   y~ = U^T y by sequential sums.  For a delta > 0: w_k = 1 / (lambda_k + delta); XWX = X~^T diag(w) X~; b = XWX^-1 X~^T diag(w) y~ by
 *   Cholesky; R = sum_k w_k (y~_k - X~_k b)^2;
 *     l(delta) = -1/2 [ (n - q) log(2 pi R / (n - q)) + sum_k log(lambda_k + delta) + log det XWX + (n - q) ]
 *   (-inf where XWX is not positive definite or R is not positive).  Search per phenotype: l at log10 delta = -5 + 0.1 i, i = 0 .. 100; the
 *   argmax (the lowest index on a tie) `best`; 40 golden-section steps on [best - 0.1, best + 0.1] clipped to [-5, 5] (ratio
 *   (sqrt(5) - 1) / 2, the inner points c < d, the interval moves to [lo, d] iff l(c) > l(d)); the best point evaluated is returned (an
 *   earlier point wins a tie), delta = pow(10, that).  Outputs per phenotype: delta, sigma_g2 = R / (n - q), sigma_e2 = delta sigma_g2,
 *   heritability = 1 / (1 + delta), l, at_boundary (log10 delta is -5 or 5), and what the device and the statistics take: weights[p] = w
 *   [n]; q + 1 rows of linear per phenotype, w o X~_0 .. w o X~_(q-1) then w o y~ ([P][q + 1][n]); M = XWX^-1 [P][q][q] (by the factor,
 *   column by column), v = M (X~^T W y~) [P][q], R [P].  The arrays are the caller's, sized for q = c_in + 1 and filled densely for the q that
 *   results.  A phenotype of which the design matrix leaves nothing (its norm 0, or its residual after centring and Q at most 2^-26 of it)
 *   gets reason 1, NaN in every scalar, in M and in v (so every statistic of it is NaN) and zero weights and linear rows.
 *   h_fixed_delta_or_null [P]: these delta are used and the search is skipped (at_boundary 0, the grid values NaN).
 *   FMH_ERR_INVALID: a NULL pointer; no phenotype, n == 0 or n > 32 768; a non-finite input, a fixed delta that is not positive;
 *   n - q - 1 < 1; P > 16 or P (q + 1) > 64.
 * fmh_lmm_stats (host only).  Per row and phenotype, a_j (j < q), b = the phenotype's q + 1 entries of lin (at p (q + 1)), d its entry of
 *   quad, c and a the row's exact counts:  aMa = sum_i (sum_j M[i][j] a_j) a_i;  D = d - aMa;  num = b - sum_j a_j v_j;  beta = num / D;
 *   rss = R - num num / D, 0 if negative;  df = n - q - 1;  se = sqrt(rss / df / D);  t = beta / se;  p = the two-sided Student-t tail of
 *   fmh_assoc_stats, that very function.  NaN in all four outputs where c = 0, a = 0, a = 2 c (the integers catch the monomorphic rows, where
 *   D would be rounding noise) or not D > 0; se == 0: t and p are NaN.  Each output may be NULL.
 * Option: FMH_LMM_ITEM_ROWS.  It changes no result, nor do FMH_GRID_PER_CU and FMH_GRID_BLOCKS.
 * Not built: leave-one-chromosome-out, low-rank relationship matrices, per-phenotype missing values, a re-fit of delta per site, logistic
 *   mixed models, sharding over devices, run_vcf wiring, u8 rows.
 */
typedef struct {
  double *h_delta, *h_sigma_g2, *h_sigma_e2, *h_heritability, *h_log_likelihood;   /* [P] */
  uint8_t *h_at_boundary, *h_reason;          /* [P]; reason: 0 fitted, 1 the design matrix leaves nothing of the phenotype */
  double *h_weights, *h_linear;               /* [P][n], [P][q + 1][n] */
  double *h_m, *h_v, *h_r;                    /* [P][q][q], [P][q], [P] */
  double* h_grid_log_likelihood_or_null;      /* [P][101]: l at the grid points; may be NULL */
} fmh_lmm_null_out;
int fmh_lmm_projections(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                        size_t row_begin, size_t row_count, const double* d_basis /* [n][K] */, size_t n_components, const double* d_weights /* [P][K] */,
                        size_t n_weights, const double* d_linear /* [L][K] */, size_t n_linear, double* d_quad /* [row_count][P] */,
                        double* d_lin /* [row_count][L] */, uint32_t* h_called_or_null, uint32_t* h_allele_count_or_null, void* stream);
int fmh_lmm_projections_host(const uint8_t* h_dosage /* [rows][n] */, size_t rows, size_t n, const double* h_basis, size_t n_components,
                             const double* h_weights, size_t n_weights, const double* h_linear, size_t n_linear, double* h_quad, double* h_lin,
                             uint32_t* h_called_or_null, uint32_t* h_allele_count_or_null);   /* host only, no device */
int fmh_lmm_null(const double* h_eigenvalues, const double* h_eigenvectors, const double* h_phenotypes, const double* h_covariates_or_null, size_t n,
                 size_t n_phenotypes, size_t n_covariates, const double* h_fixed_delta_or_null /* [P] */, size_t* h_q,
                 uint8_t* h_dropped_or_null /* [n_covariates] */,
                 const fmh_lmm_null_out* out);   /* host only, no device */
int fmh_lmm_stats(const double* h_quad, const double* h_lin, const uint32_t* h_called, const uint32_t* h_allele_count, size_t n_rows,
                  const double* h_m, const double* h_v, const double* h_r, uint64_t n_samples, size_t q, size_t n_phenotypes, double* h_beta,
                  double* h_se, double* h_t, double* h_p);   /* host only, no device */

/* ---- admixture: ancestry proportions by EM (an addition: the reference has none) -----------------------------------------------------------------
 * The model of ADMIXTURE, FRAPPE, fastmixture and STRUCTURE: per sample the proportions Q of K ancestral populations, per site the allele
 * frequencies F of those populations.  The project's own definition.
 *
 * Selected diploid samples i = 0 .. n-1 (a list as fmh_grm takes it); kept rows = a row range and an optional keep mask, as fmh_grm's.  Genotype
 * classes are fmh_grm's codes: g in {0, 1, 2}, or not called (a missing call, or an allele above 1).  c_r = the called genotypes of row r, a_r
 * the alternate alleles among them; a row is USABLE when c_r > 0 and 0 < a_r < 2 c_r; every other row is reported and takes no part.  m_i = the
 * number of usable rows at which sample i is called.  Usable rows are j = 0 .. m-1 in row order.
 *
 * State: Q [n][K] and F [m][K], f64, row-major, 1 <= K <= 16 (FMH_ADMIX_MAX_K); G = fl(1 - F) elementwise; eps = 1e-5 (ADMIXTURE's bound).
 * One EM step (Q, F) -> (Q', F'), every sum over called genotypes only:
 *   h0_ij = sum_k q_ik f_jk        h1_ij = sum_k q_ik g_jk      (two sums of positive terms; 1 - h0 is never formed)
 *   u_ij  = g_ij / h0_ij           v_ij  = (2 - g_ij) / h1_ij
 *   A_jk  = sum_i u_ij q_ik        B_jk  = sum_i v_ij q_ik
 *   f'_jk = clamp(f_jk A_jk / (f_jk A_jk + g_jk B_jk), eps, 1 - eps)
 *   E_ik  = sum_j (u_ij f_jk + v_ij g_jk)
 *   q0_ik = clamp(q_ik E_ik / (2 m_i), eps, 1 - eps);   q'_ik = q0_ik / sum_k q0_ik   (k ascending)
 *   l(Q, F) = sum_ij g_ij log h0_ij + (2 - g_ij) log h1_ij       (of the step's INPUT)
 * A sample with m_i = 0 keeps its row of Q.  Flag bits FMH_ADMIX_UPDATE_Q and FMH_ADMIX_UPDATE_F: a half whose bit is clear is copied to the
 * output unchanged; FMH_ADMIX_UPDATE_Q alone is projection (new samples on a reference panel's frequencies).  K = 1 has the closed form
 * f' = a / (2 c) up to rounding and q' = 1.  sum_k q_ik E_ik = 2 m_i, and l does not fall from step to step.
 *
 * fmh_admix is an opaque handle, because a fit reads the same genotypes hundreds of times.  fmh_admix_create counts c, a through
 * fmh_genotype_counts, marks the usable rows, builds their 2-bit code image (sample-major, fmh_grm's) and computes m_i; the handle owns its
 * device memory and does not need the matrix afterwards.  Refusals come before any launch: FMH_ERR_INVALID for NULLs, n_samples == 0, bad
 * lists or ranges; FMH_ERR_UNSUPPORTED with a message for ploidy != 2, for a matrix without the packed image, and for an image over
 * FMH_ADMIX_BUDGET_BYTES.  No kept row or no usable row gives a handle with m = 0, whose step is FMH_OK and writes only Q' (copied) and l = 0.
 * fmh_admix_info: n, the kept rows, m, and host arrays owned by the handle: usable, called, allele_count per KEPT row, sample_sites [n].
 *
 * fmh_admix_step: d_q [n][K], d_f [m][K] in, d_q_out, d_f_out out (device; input and output must not alias: refused).  Every output entry is
 * WRITTEN by one writer; nothing need be zeroed by the caller; there are no floating-point atomics, and two runs give the same bits.  K
 * outside 1 .. 16 and NULLs are refused.  Inputs outside [eps, 1 - eps] (or rows of Q that do not sum to one) are the caller's affair: nothing
 * checks them.  h_loglik_or_null == NULL runs a kernel without logarithms; Q', F' have the same bits either way.  The call synchronises the
 * stream.  The step runs on v_mfma_f64_16x16x4_f64 for every K; a workgroup owns a block of usable rows
 * (FMH_ADMIX_ITEM_ROWS, rounded up to whole passes of 128 rows; default: two blocks per compute unit, fewer where the slabs would pass the
 * budget).  FMH_ADMIX_BUDGET_BYTES (default 4 GiB) bounds image plus padded state plus slabs; more is refused with the bytes needed.  The
 * item size may change the last bits of Q' and l (the order of a sum) and no bit of F'; FMH_GRID_PER_CU and FMH_GRID_BLOCKS change no bit.
 *
 * Host only, no device:
 *   fmh_admix_step_host: the twin for CPU tests.  h_dosage u8 [rows][n] (0, 1, 2; above 2 = not called); the same usable rule; h_f, h_f_out
 *     [m][K] over the usable rows; every sum over ascending index in plain f64 (rows outer, samples inner for A, B, E and l).  `tracks` (may be
 *     NULL, each member may be NULL) receives usable, called, allele_count per row, sample_sites [n] and m.  With all four state pointers NULL
 *     only the tracks are computed (how a caller learns m).
 *   fmh_admix_start: the default start.  mix = splitmix64's finaliser after adding 0x9E3779B97F4A7C15; U(t) = (mix(mix(seed) + t) >> 11) 2^-53;
 *     q_ik = w_ik / sum_k w_ik with w = 1 + U(i K + k); f_jk = clamp(a_j / (2 c_j) + 0.2 (U(2^40 + j K + k) - 0.5), 0.01, 0.99); c, a of the m
 *     usable rows.
 *   fmh_admix_accelerate: the extrapolation of one SQUAREM-S3 cycle.  r = t1 - t0, v = (t2 - t1) - r, alpha = max(1, sqrt(sum r^2 / sum v^2)),
 *     the sums over Q then F in ascending index; ta = (t0 + (2 alpha) r) + (alpha alpha) v, then F clamped to [eps, 1 - eps], Q clamped and
 *     renormalised as in the step.  sum v^2 == 0: ta = t2 and *h_alpha = 0 (nothing to extrapolate).  m = 0 leaves F out (projection).
 *   The accelerated cycle a caller runs with these: t1 = M(t0) gives l0, t2 = M(t1) gives l1, ta from fmh_admix_accelerate, t3 = M(ta) gives
 *   la; the next cycle starts from t3 if la is finite and la >= l1, else from t2 (and from t2 without a third step when alpha = 0).  The l0 of
 *   successive cycles never falls.
 *
 * Not built: K > 16; a VALU route for small K; the extrapolation on the device; cross-validation error; supervised ancestry; bootstrap or
 * standard errors; alignment of component labels between runs; mini-batch updates; haploid data; sharding over devices; run_vcf wiring; u8 rows. */
#define FMH_ADMIX_MAX_K 16
#define FMH_ADMIX_UPDATE_Q 1u
#define FMH_ADMIX_UPDATE_F 2u
typedef struct fmh_admix fmh_admix;
typedef struct {
  uint64_t n_samples, kept_rows, usable_rows;
  const uint8_t* h_usable;             /* [kept_rows]; owned by the handle, as the three below */
  const uint32_t *h_called, *h_allele_count;   /* [kept_rows] */
  const uint64_t* h_sample_sites;      /* [n_samples] m_i */
} fmh_admix_info_out;
typedef struct {
  uint8_t* h_usable;                   /* [rows] */
  uint32_t *h_called, *h_allele_count; /* [rows] */
  uint64_t* h_sample_sites;            /* [n] */
  uint64_t* h_usable_rows;             /* m */
} fmh_admix_tracks;
int fmh_admix_create(const fmh_matrix* m, const uint32_t* h_samples_or_null /* ascending, distinct; NULL = the first n_samples */, size_t n_samples,
                     size_t row_begin, size_t row_count, const uint8_t* h_keep_or_null /* [row_count] */, fmh_admix** out, void* stream);
int fmh_admix_info(const fmh_admix* h, fmh_admix_info_out* info);
void fmh_admix_destroy(fmh_admix* h);
int fmh_admix_step(const fmh_admix* h, size_t n_components, const double* d_q, const double* d_f, double* d_q_out, double* d_f_out,
                   double* h_loglik_or_null, uint32_t flags, void* stream);
int fmh_admix_step_host(const uint8_t* h_dosage /* [rows][n] */, size_t rows, size_t n, size_t n_components, const double* h_q, const double* h_f,
                        double* h_q_out, double* h_f_out, double* h_loglik_or_null, uint32_t flags,
                        const fmh_admix_tracks* tracks_or_null);   /* host only, no device */
int fmh_admix_start(const uint32_t* h_called, const uint32_t* h_allele_count, size_t m, size_t n, size_t n_components, uint64_t seed, double* h_q,
                    double* h_f);   /* host only, no device */
int fmh_admix_accelerate(const double* h_q0, const double* h_f0, const double* h_q1, const double* h_f1, const double* h_q2, const double* h_f2,
                         size_t n, size_t m, size_t n_components, double* h_qa, double* h_fa, double* h_alpha);   /* host only, no device */

/* ---- haplotype homozygosity windows: Garud's H (an addition: the reference has none) -------------------------------------------
 * Which haplotypes are identical over a stretch of sites, from the bit-packed image.
 * A group is a 0/1 column mask with n >= 1 members (fmh_groups); members are ranked 0 .. n-1 by ascending column.  A window is a row range
 * [begin, end).  An entry's STATE is `uncalled`, or its allele 0 .. 7 when called.  Bits of the allele planes under uncalled entries are
 * undefined (fmh_matrix_create_packed accepts junk there): every plane is masked with the called plane, as for the spectra.
 * Two members are IDENTICAL IN A WINDOW iff their states are equal at every row of the window: two uncalled entries are equal, an uncalled
 * entry and a called one are not (scikit-allel's convention of treating -1 as a value).  The classes of this equivalence have sizes
 * c_1 >= c_2 >= c_3 >= ...; they sum to n and there are K of them.  An empty window has one class of size n.
 * Per window the device produces integers only, a record fmh_hap_window:
 *   sum_sq = sum_i c_i^2     distinct = K     top[0..2] = c_1, c_2, c_3 (0 where K is smaller)
 * and, when d_first is given, the partition itself in canonical form: d_first[w][i] = the rank of the FIRST (lowest-ranked) member
 * identical to member i in window w - so d_first[w][i] <= i, == i exactly for one member of each class, and two members are identical iff
 * their entries are equal.  Results never depend on an option, the grid or the order in which anything ran.
 *
 * fmh_haplotype_windows: ONE group over n_windows row ranges [h_windows[2w], h_windows[2w+1]) of the matrix.  Ranges may overlap, be empty
 *   and come in any order; begin <= end <= variants.  d_out [n_windows] and d_first_or_null [n_windows][n] u32 are on the matrix's device
 *   and need not be zeroed: every entry is written.  The call enqueues on `stream` and synchronises it.
 * Refusals, before any device work, in this order: a NULL matrix, groups, windows or d_out pointer; a group count other than 1; groups that
 * were not made for this matrix; a group with no member; a window outside the matrix or with begin > end; n_windows == 0 - all
 * FMH_ERR_INVALID; then n > fmh_haplotype_max_members() (the message names the cap); n_windows * n above 2^32 entries when d_first is
 * given; a matrix without the packed image (call fmh_matrix_pack first) - FMH_ERR_UNSUPPORTED.
 * fmh_haplotype_max_members (needs no device): the largest group the kernel takes, 34 304 - the partition of a window lives in the 160 KiB
 *   of LDS of one compute unit, 4.75 bytes per member plus a 512-byte head.  A device that gives a workgroup less LDS than a group needs
 *   refuses that group with FMH_ERR_UNSUPPORTED.
 * Option: FMH_HAP_THREADS = 64 | 256 | 512 | 1024 threads per workgroup (other values count as unset).  Default, by measurement: 64 up to 256
 * members; with at least one window per compute unit 256 up to 8 192 members, 512 up to 16 384, 1 024 beyond; with fewer windows than
 * compute units 256 up to 1 024 members, 512 up to 4 096, 1 024 beyond.  FMH_GRID_PER_CU / FMH_GRID_BLOCKS size the persistent grid as for
 * the sweeps.
 * None changes a result.
 *
 * fmh_haplotype_stats (host only, no device): the statistics of n_windows records of a group of n members (1 <= n < 2^26).  Each value is
 * ONE f64 division of two integers, both below 2^53 and converted exactly, so the quotient is the correctly rounded one:
 *   h1 = sum_sq / n^2                                  (haplotype homozygosity)
 *   h12 = (sum_sq + 2 c1 c2) / n^2                     (the two largest classes pooled)
 *   h123 = (sum_sq + 2 (c1 c2 + c1 c3 + c2 c3)) / n^2  (the three largest pooled)
 *   h2_h1 = (sum_sq - c1^2) / sum_sq
 *   haplotype_diversity = (n^2 - sum_sq) / (n (n - 1)),  NaN when n == 1
 * A record with sum_sq == 0 or sum_sq > n^2, c1^2 > sum_sq or c1 + c2 + c3 > n is no partition of n members: FMH_ERR_INVALID.
 */
typedef struct { uint64_t sum_sq;            /* sum of c_i^2 */
                 uint32_t distinct;          /* K */
                 uint32_t top[3];            /* c_1, c_2, c_3; 0 where K is smaller */ } fmh_hap_window;   /* 24 bytes */
typedef struct { double h1, h12, h123, h2_h1, haplotype_diversity; } fmh_hap_stats_out;

int fmh_haplotype_windows(const fmh_matrix* m, const fmh_groups* g /* exactly 1 group */, const uint64_t* h_windows /* [n_windows][2] */,
                          size_t n_windows, fmh_hap_window* d_out /* [n_windows] */, uint32_t* d_first_or_null /* [n_windows][n] */,
                          void* stream);
int fmh_haplotype_stats(const fmh_hap_window* h_windows, size_t n_windows, uint64_t n, fmh_hap_stats_out* h_out);   /* host only, no device */
uint32_t fmh_haplotype_max_members(void);   /* the largest group the kernel takes; needs no device */

/* ---- extended haplotype homozygosity scans: the integers behind iHS and nSL (an addition: the reference has none) -----------------
 * How far identity extends around a site.  Matrix, group (exactly one, n members), member ranks and an entry's STATE are those of
 * fmh_haplotype_windows: uncalled, or allele 0 .. 7 under the called plane; two uncalled entries are equal.
 * Per call: a row range [row_begin, row_end) that no scan leaves; h_focal[n_focal], u64 rows inside the range, in any order, repeats
 * allowed; h_positions_or_null[variants] u32, non-decreasing over the range - x(r) = h_positions[r], NULL means x(r) = r; and
 * fmh_ehh_params: min_ehh_num / min_ehh_den (den >= 1, num <= den; num == 0 = no threshold), max_extent (0 = unlimited), max_gap (0 = none),
 * min_core.
 * CORE CLASSES of focal row f: core 0 = the members whose state at f is called allele 0, core 1 = those with called allele 1; every other
 * member (uncalled, allele >= 2) belongs to neither and counts nowhere.  n_a = the size of core a, P_a(0) = n_a (n_a - 1) / 2.
 * PAIR COUNTS: for side s in {-1 (left), +1 (right)} and d >= 1, r_d = f + s d; P_a(d) = the number of unordered pairs of core-a members
 * whose states agree at every row f, r_1, .., r_d.  Every flanking row counts whatever it holds (uncalled and alleles >= 2 are states).
 * STOP RULES, per side and core, with alive_a = P_a(0) > 0 and gap_d = |x(r_d) - x(r_{d-1})| (r_0 = f): for d = 1, 2, .. while a core is
 * alive, d <= max_extent (when that is not 0) and r_d is inside the range, for each alive a in this order:
 *   1. if max_gap > 0 and gap_d > max_gap: flag GAP_a, the core is finished;
 *   2. else if P_a(d) den < P_a(0) num: the core is finished (the normal end; the step is not counted);
 *   3. else area2_a += (P_a(d-1) + P_a(d)) gap_d, pair_steps_a += P_a(d), steps_a = d; if P_a(d) == 0 the core is finished.
 * A core still alive when the loop ends gets flag EDGE_a.  If min(n_0, n_1) < min_core the item writes flag SKIPPED, zeros and n_0, n_1
 * and scans nothing.  All products fit u64: P < 2^30, den < 2^32, the span of positions < 2^32, area2 <= 2 P(0) span < 2^63.
 * The record fmh_ehh_side, one per (focal, side), d_out[n_focal][2] with the left side first (56 bytes), is integers only; optional
 * d_pairs_or_null[n_focal][2 sides][2 cores][max_extent] u32: entry d-1 holds P_a(d) for 1 <= d <= steps_a, every other entry is 0.  Every
 * entry of both is written: nothing needs zeroing beforehand.  Results never depend on an option, the grid, the thread count or the order
 * in which anything ran.  The call enqueues on `stream` and synchronises it.
 *
 * Refusals of fmh_ehh_scan, before any device work, in this order: a NULL matrix, groups, h_focal, params or d_out pointer; a group count
 * other than 1; groups that were not made for this matrix; a group with no member; row_begin > row_end or row_end > variants; a focal row
 * outside the range; n_focal == 0; min_ehh_den == 0; min_ehh_num > min_ehh_den; positions that descend inside the range; d_pairs given
 * with max_extent == 0 - all FMH_ERR_INVALID; then n > fmh_ehh_max_members() (the message names the cap); d_pairs above 2^32 entries; a
 * matrix without the packed image (call fmh_matrix_pack first) - FMH_ERR_UNSUPPORTED.
 * fmh_ehh_max_members (needs no device): 34 304, the cap of fmh_haplotype_windows - the scan keeps the same state per member in LDS (one
 *   u32: the label, and in turn the parked row state and the class size) and needs nothing more.
 * Options: FMH_HAP_THREADS, FMH_GRID_PER_CU and FMH_GRID_BLOCKS as for fmh_haplotype_windows, with items (focal, side) in place of windows.
 *
 * fmh_ehh_stats (host only, no device): per focal, from its two records and for a in {0, 1}:
 *   ihh_a = (double)(area2_L + area2_R) / (double)(2 P_a(0))
 *   sl_a  = (double)(P_a(0) + pair_steps_L + pair_steps_R) / (double)P_a(0)
 * each two exact-or-correctly-rounded u64 -> f64 conversions and one division; then ihs = log(ihh_1 / ihh_0), nsl = log(sl_1 / sl_0).
 * ihh_a and sl_a are NaN where P_a(0) == 0, where the item is SKIPPED, and - unless include_edges != 0 - where any EDGE or GAP flag of
 * either side and core is set; ihs and nsl are NaN where one of their operands is NaN or 0.  Two records of a focal that disagree in
 * core[] or in SKIPPED are FMH_ERR_INVALID.
 */
#define FMH_EHH_EDGE0 1u     /* core 0 was still alive at max_extent or at the end of the range */
#define FMH_EHH_EDGE1 2u
#define FMH_EHH_GAP0 4u      /* core 0 met a gap above max_gap */
#define FMH_EHH_GAP1 8u
#define FMH_EHH_SKIPPED 16u  /* min(n_0, n_1) < min_core: nothing was scanned */
typedef struct { uint32_t min_ehh_num, min_ehh_den;   /* the threshold num / den on P(d) / P(0); num == 0 = none */
                 uint32_t max_extent;                 /* rows a side may walk; 0 = unlimited */
                 uint32_t max_gap;                    /* 0 = none */
                 uint32_t min_core;
                 uint32_t reserved;                   /* 0 */ } fmh_ehh_params;
typedef struct { uint64_t area2[2];        /* per core: sum of (P(d-1) + P(d)) gap_d over the counted steps */
                 uint64_t pair_steps[2];   /* per core: sum of P(d) over the counted steps */
                 uint32_t steps[2];        /* per core: the last counted d */
                 uint32_t core[2];         /* n_0, n_1 */
                 uint32_t flags;           /* FMH_EHH_* */
                 uint32_t reserved;        /* 0 */ } fmh_ehh_side;   /* 56 bytes */
typedef struct { double ihh[2], sl[2], ihs, nsl; } fmh_ehh_stats_out;

int fmh_ehh_scan(const fmh_matrix* m, const fmh_groups* g /* exactly 1 group */, size_t row_begin, size_t row_end,
                 const uint64_t* h_focal /* [n_focal] */, size_t n_focal, const uint32_t* h_positions_or_null /* [variants] */,
                 const fmh_ehh_params* params, fmh_ehh_side* d_out /* [n_focal][2] */,
                 uint32_t* d_pairs_or_null /* [n_focal][2][2][max_extent] */, void* stream);
int fmh_ehh_stats(const fmh_ehh_side* h_sides /* [n_focal][2] */, size_t n_focal, int include_edges,
                  fmh_ehh_stats_out* h_out /* [n_focal] */);   /* host only, no device */
uint32_t fmh_ehh_max_members(void);   /* the largest group the scan takes; needs no device */

/* ---- multi-GPU: region sharding + RCCL reduce of the regional accumulators -------------------------------- */
/*
 * Sites are independent: rank r of G sweeps only its contiguous slab of the region and writes its own
 * per-site tracks; the only exchange is the SUM of the regional accumulators - what the reference's rayon fold/reduce
 * does across its worker threads (stats.rs:1365-1461 for the summaries, the serial sums of 1554-1623 and 2145-2374
 * for Hudson and W&C).  A communicator carries that sum over RCCL (xGMI inside a node): one ncclAllReduce per vector
 * type, a few hundred bytes, latency-bound.  RCCL is bound at run time (dlopen), so single-GPU hosts never load it.
 * Integer totals are exact; f64 totals depend on the reduction order (1e-9 contract, as with rayon).
 *
 *   one process per GPU (MPI / torch.distributed.run):  rank 0 calls fmh_comm_get_unique_id, ships the 128 bytes to the
 *     other ranks over any channel, every rank calls fmh_comm_init_rank.
 *   one process, several GPUs (run_vcf --devices):       fmh_comm_init_all; each device's thread then uses its own handle
 *     concurrently.  When a device appears more than once in the list (rehearsal on a one-GPU box) or
 *     FMH_COMM_TRANSPORT=host is set, the handles share an in-process rendezvous that sums in rank order on the host
 *     instead - RCCL cannot place two ranks on one GPU.
 */
typedef struct fmh_comm fmh_comm;
#define FMH_COMM_ID_BYTES 128
int fmh_comm_get_unique_id(void* h_id /*[FMH_COMM_ID_BYTES]*/);
int fmh_comm_init_rank(const void* h_id, int world, int rank, int device, fmh_comm** out);
int fmh_comm_init_all(const int* h_devices, int n, fmh_comm** h_out /*[n]*/);
/* A communicator of ONE rank that needs no transport (and no RCCL): what a single GPU uses for the pipelined
 * fmh_hudson_sweep_sharded_begin / _end calls when it scans many windows. */
int fmh_comm_init_local(int device, fmh_comm** out);
int fmh_comm_destroy(fmh_comm* c);
/* transport: 0 = RCCL, 1 = in-process host rendezvous, 2 = local (one rank, nothing to exchange) */
int fmh_comm_info(const fmh_comm* c, int* world, int* rank, int* device, int* transport);
/* One line for reports: "transport=rccl world=8 rank=3 device=3 rccl_library=<file the process bound> rccl_version=<ncclGetVersion> ..." */
int fmh_comm_describe(const fmh_comm* c, char* h_text, size_t cap);
/* For a rank that FAILED before its collective (allocation, upload, validation): wakes the peers of an in-process group, which return
 * FMH_ERR_INVALID from the collective they are waiting in instead of blocking for ever, and aborts the RCCL communicator
 * (ncclCommAbort).  The communicator only accepts fmh_comm_destroy afterwards.  Every sharded _begin validates its arguments before
 * it enqueues anything, so a rank whose _begin returned an error has not entered the collective and may call this. */
int fmh_comm_abort(fmh_comm* c);

/* Element-wise sum over all ranks, in place, blocking (collective: every rank calls it with the same lengths;
 * n_f64, n_u64 <= FMH_COMM_MAX_VALUES). */
#define FMH_COMM_MAX_VALUES 512
int fmh_allreduce_totals(fmh_comm* c, double* h_f64, size_t n_f64, uint64_t* h_u64, size_t n_u64);
/* The same in two halves: _begin enqueues the reduce on the communicator's own stream and returns, _end waits for it
 * and writes the sums.  One reduce may be in flight per communicator. */
int fmh_allreduce_totals_begin(fmh_comm* c, const double* h_f64, size_t n_f64, const uint64_t* h_u64, size_t n_u64);
int fmh_allreduce_totals_end(fmh_comm* c, double* h_f64, uint64_t* h_u64);

/*
 * Region-sharded Hudson sweep: this rank's rows [row_begin, row_begin + row_count) of ITS slab matrix, then the sum of the
 * regional accumulators over all ranks - fmh_hudson_sweep + fmh_allreduce_totals without a host hop in between: the
 * partials are finalised on the device, reduced there by RCCL on the communicator's stream and land in pinned memory.
 * _begin returns as soon as the work is enqueued (up to FMH_SHARDED_IN_FLIGHT sweeps per communicator), _end waits for
 * the OLDEST outstanding one and returns its region-wide totals (pop[].haplotype_capacity is the local mask popcount,
 * identical on every rank).  A loop `begin(k); if (k) end(k-1)` overlaps the reduce of one window with the sweep of the
 * next, which is what keeps small slabs (1.25 M sites x 5 000 haplotypes is 0.16 ms of kernel) from paying the
 * collective's latency; keeping two or three sweeps ahead (`begin(k); if (k >= 2) end(k-2)`) also covers a reduce that can only
 * start once a persistent sweep grid frees compute units, or that takes longer than one sweep.  fmh_hudson_sweep_sharded = _begin + _end.
 */
#define FMH_SHARDED_IN_FLIGHT 4
int fmh_hudson_sweep_sharded_begin(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                                   int formula, const fmh_hudson_sites* sites_or_null, void* stream);
int fmh_hudson_sweep_sharded_end(fmh_comm* c, fmh_hudson_totals* h_global_totals);
int fmh_hudson_sweep_sharded(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                             int formula, const fmh_hudson_sites* sites_or_null, fmh_hudson_totals* h_global_totals, void* stream);

/*
 * The same pipeline for the other two regional reductions north_star names ("RCCL reduce ... for the sum-a / sum-b and global pi
 * accumulators"): sweep -> finalise on the device -> grouped ncclAllReduce of the 64 + 64 accumulators on the communicator's stream ->
 * one D2H; no host hop, FMH_SHARDED_IN_FLIGHT sweeps of ANY kind may be in flight per communicator and each _end collects the oldest
 * (it must be of its kind).  W&C: calculate_overall_fst_wc's sums (stats.rs:2145-2374) - two to eight groups run as one fused kernel (five
 * to eight: with alleles up to 3); more than 3 alleles with five to eight groups, or rows too wide for all masks, run the blocking fmh_wc_sweep
 * inside _begin and only the reduce is pipelined.
 * Population summaries: build_dense_population_summary's scalars (stats.rs:1367-1470) for up to FMH_MAX_GROUPS populations.
 * Per-site tracks stay on the rank that owns the rows; haplotype_capacity is the local mask popcount (identical on every rank).
 */
int fmh_wc_sweep_sharded_begin(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, double* d_a,
                               double* d_b, uint8_t* d_state, uint32_t* d_group_called, void* stream);
int fmh_wc_sweep_sharded_end(fmh_comm* c, fmh_wc_totals* h_global_totals);
int fmh_wc_sweep_sharded(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, double* d_a, double* d_b,
                         uint8_t* d_state, uint32_t* d_group_called, fmh_wc_totals* h_global_totals, void* stream);
int fmh_population_summaries_sharded_begin(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count,
                                           int formula, uint32_t* d_alt, uint32_t* d_called, void* stream);
int fmh_population_summaries_sharded_end(fmh_comm* c, fmh_pop_totals* h_global_totals /*[n_groups]*/);
int fmh_population_summaries_sharded(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, int formula,
                                     uint32_t* d_alt, uint32_t* d_called, fmh_pop_totals* h_global_totals, void* stream);
/* fmh_pair_region_sweep over this rank's slab, totals (population summaries + Hudson) summed over the ranks the same way; collected by
 * fmh_hudson_sweep_sharded_end (the totals struct is the same) */
int fmh_pair_region_sweep_sharded_begin(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, int summary_formula,
                                        int hudson_formula_or_negative, const fmh_pair_diversity_sites* diversity_or_null,
                                        const fmh_hudson_sites* sites_or_null, void* stream);
int fmh_pair_region_sweep_sharded(fmh_comm* c, const fmh_matrix* m, const fmh_groups* g, size_t row_begin, size_t row_count, int summary_formula,
                                  int hudson_formula_or_negative, const fmh_pair_diversity_sites* diversity_or_null,
                                  const fmh_hudson_sites* sites_or_null, fmh_hudson_totals* h_global_totals, void* stream);

/*
 * The PCA Gram (fmh_pca_gram) of a cohort whose SITES are spread over the ranks - the Gram is a plain sum over sites, and the only
 * O(n^2 m) step of the PCA.  Every rank passes ITS slab matrix (same samples, ploidy 2) and the kept rows of that slab (row indices
 * local to the slab) with their set / clear values; n_kept may be 0 on a rank (it contributes zeros).  On return every rank's
 * d_gram[n][n] (n = samples * 2, on the communicator's device) holds the sum over the ranks of Z_r Z_r^T / (n - 1).
 *
 * How: the local Gram is fmh_pca_gram's own path; only the upper triangle travels (n (n + 1) / 2 doubles, row i at offset
 * i n - i (i - 1) / 2), and the full matrix is rebuilt from the summed triangle with (i, j) and (j, i) written from the same value - so the
 * result is exactly symmetric on every transport.  Local communicator: nothing is exchanged.  In-process transport: the triangles are
 * added on the host in rank order, so every rank ends with the same bits and two calls give the same bits.  RCCL: one ncclAllReduce
 * (f64, sum) on the communicator's stream, ordered behind the pack and before the unpack by events; the order of RCCL's additions is
 * RCCL's, so run-to-run bits are NOT promised there with more than one rank.  A communicator of one rank gives fmh_pca_gram's bits
 * (zeros for n_kept == 0) on every transport.
 *
 * Collective: every rank calls it.  Every argument and the memory budget are checked BEFORE anything is enqueued, so a rank whose call
 * returned FMH_ERR_INVALID / FMH_ERR_UNSUPPORTED from those checks has not entered the collective and may call fmh_comm_abort to
 * release its peers.  On the in-process transport ranks whose matrices differ in sample count get FMH_ERR_INVALID from the collective
 * (it compares the lengths), not a wrong sum.  No other collective may be in flight on the communicator.
 *
 * Device memory: what fmh_pca_gram takes plus the packed triangle, 4 n (n + 1) bytes from the library's pool; the sum must stay
 * within FMH_PCA_BUDGET_BYTES, else FMH_ERR_UNSUPPORTED.  The in-process transport also holds one triangle per rank plus the sum in
 * host memory.  This reduce is not bound by FMH_COMM_MAX_VALUES (that is fmh_allreduce_totals' limit).  Synchronises `stream`.
 */
int fmh_pca_gram_sharded(fmh_comm* c, const fmh_matrix* m, const uint64_t* h_kept_rows, size_t n_kept, const double* h_set_value,
                         const double* h_clear_value, double* d_gram /* n x n, n = samples * 2 */, void* stream);

/*
 * Packing of the totals structs into the f64 + u64 vectors a sum-reduce moves (fmh_allreduce_totals, or MPI / any other
 * transport).  Everything packed is a plain sum over slabs, except haplotype_capacity / sites_attempted-style constants,
 * which unpack restores from the rank count carried in the last u64 slot.
 */
#define FMH_HUDSON_PACK_F64 10
#define FMH_HUDSON_PACK_U64 10
int fmh_hudson_totals_pack(const fmh_hudson_totals* t, double* h_f64 /*[FMH_HUDSON_PACK_F64]*/,
                           uint64_t* h_u64 /*[FMH_HUDSON_PACK_U64]*/);
int fmh_hudson_totals_unpack(fmh_hudson_totals* t, const double* h_f64, const uint64_t* h_u64);
/* per-population summaries (fmh_population_summaries, fmh_diversity_sites): n entries -> n f64 (pi_sum) and 3n + 1 u64
 * (segregating, uncallable, haplotype_capacity per population, then the rank count) */
#define FMH_POP_PACK_F64(n) ((size_t)(n))
#define FMH_POP_PACK_U64(n) (3 * (size_t)(n) + 1)
int fmh_pop_totals_pack(const fmh_pop_totals* t, int n, double* h_f64, uint64_t* h_u64);
int fmh_pop_totals_unpack(fmh_pop_totals* t, int n, const double* h_f64, const uint64_t* h_u64);
/* W&C regional sums (calculate_overall_fst_wc, stats.rs:2145-2374): slots = 1 + n_groups (n_groups - 1) / 2 ->
 * 2 * slots f64 (sum_a, sum_b) and slots + 1 u64 (informative_sites per slot, sites_attempted) */
#define FMH_WC_PACK_F64(slots) (2 * (size_t)(slots))
#define FMH_WC_PACK_U64(slots) ((size_t)(slots) + 1)
int fmh_wc_totals_pack(const fmh_wc_totals* t, int n_groups, double* h_f64, uint64_t* h_u64);
int fmh_wc_totals_unpack(fmh_wc_totals* t, int n_groups, const double* h_f64, const uint64_t* h_u64);

/* ---- measurement ---------------------------------------------------------------------------------- */
/* Accumulated HIP-event time (ms) and launch count of the dominant sweep kernel since the last
 * reset, measured on the stream the kernel ran on.  Timing is off unless enabled: the two event
 * records of a timed launch cost a few microseconds of stream time.  fmh_timing_enable(n) with
 * n > 1 times every n-th sweep only (the launch count returned is that of the timed ones). */
int fmh_timing_enable(int on);
int fmh_timing_reset(void);
int fmh_timing_read(double* h_total_ms, uint64_t* h_launches);
/* shortest and longest of the launches timed since the last reset (0, 0 when none) */
int fmh_timing_read_minmax(double* h_min_ms, double* h_max_ms);
/* The same for the grouped all-reduce of the timed sharded sweeps (RCCL transport): HIP events on the communicator's stream around
 * ncclGroupStart .. ncclGroupEnd - the device-side latency of one 2 x 512-byte reduce. */
int fmh_timing_read_reduce(double* h_total_ms, uint64_t* h_reduces);
int fmh_timing_reset_reduce(void);
/* PCA stage times of the calling thread while timing was enabled, ms by HIP events: [0..2] gather + transpose, Gram, split-K reduce of
 * the last fmh_pca_gram; [3] the kernel of the last fmh_pca_scan_sites; [4] the eigen solver of the last fmh_pca_eigen_scores
 * (rocsolver_dsyevd by events, the host solver by the host clock); [5] which solver that was (1 = host, 2 = rocSOLVER; set always). */
int fmh_timing_read_pca(double* h_stage_ms /*[6]*/);
/* A measurement aid (tools/measure_kinship.py), inert unless timing is enabled: stage times of the calling thread's last fmh_pairwise_differences or fmh_kinship_counts while timing was enabled, ms by HIP events,
 * summed over the call's row slabs: [0] the planes kernels, [1] the first Gram of a slab with its slab reduce (pairwise: all its Grams;
 * kinship: the stacked [H; V] or H operand), [2] the second Gram (kinship: W), [3] the finish kernel. */
int fmh_timing_read_gram(double* h_stage_ms /*[4]*/);
/* Stage times of the calling thread's last fmh_grm while timing was enabled, ms by HIP events: [0] the codes kernel (with the plane flags),
 * [1] the Gram, [2] the slab reduce and the addition into the caller's matrix.  (Its eigen solver is fmh_timing_read_pca's [4].) */
int fmh_timing_read_grm(double* h_stage_ms /*[3]*/);
/* Stage times of the calling thread's last fmh_admix_step while timing was enabled, ms by HIP events: [0] the padded copies of Q and F,
 * [1] the step kernel, [2] the reduce kernel (Q' and the log-likelihood). */
int fmh_timing_read_admix(double* h_stage_ms /*[3]*/);

#ifdef __cplusplus
}
#endif
#endif /* FERROMIC_HIP_H */
