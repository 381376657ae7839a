// abi_internal.hpp — host-side internals shared by the translation units of libferromic_hip.so (abi.hip, sweep_dispatch.hip,
// pairwise.hip, comm.hip and the sweep_*.hip files that hold the kernel instantiations).  Nothing here is part of the C-ABI: the library
// is built with -fvisibility=hidden and only include/ferromic_hip.h's functions are exported.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/ferromic_hip.h"
#pragma GCC visibility pop

#include "sweep_kernels.hpp"

namespace fmhi {

// ---- errors: status code + thread-local message (fmh_last_error) ----------------------------------------------------
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return ::fmhi::fail(_e == hipErrorNoDevice ? FMH_ERR_NO_DEVICE : FMH_ERR_HIP, "%s: %s (%s:%d)", \
                          #expr, hipGetErrorString(_e), __FILE__, __LINE__);                        \
  } while (0)

#define FMH_TRY(expr)            \
  do {                           \
    int _s = (expr);             \
    if (_s != FMH_OK) return _s; \
  } while (0)

int use_device(int device);  // range check + hipSetDevice

// ---- device memory pool (abi.hip) -------------------------------------------------------------------------------------
hipError_t pool_malloc(int device, void** out, size_t bytes);
void pool_free(int device, void* p);
void pool_trim(int device);

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- per-process options (fmh_set_option / fmh_get_option, abi.hip) ------------------------------------------------------
// Every switch that routes a kernel or sizes a launch lives here as an atomic integer.  The FMH_* environment is read ONCE, when the
// library first needs an option (so `FMH_LAYOUT=bytes python ...` and a child process started with such an environment still work);
// after that only fmh_set_option changes a value.  Nothing on a launch path reads the environment: round 2 read ten variables per enqueue, which
// cost 1-2 us per sweep and raced with any host thread calling setenv.
struct Options {
  std::atomic<long long> layout_bytes{0};        // FMH_LAYOUT = bytes | packed: keep the u8 kernels on matrices that still hold their byte rows
  std::atomic<long long> mask_mode{-1};          // FMH_MASK_MODE: force a slower mask route (tests / measurements)
  std::atomic<long long> defer_tiles{0};         // FMH_DEFER_TILES: 1..16 forces the deferral depth (1 = undeferred); 0 = by the launch size
  std::atomic<long long> packed_lpr{0};          // FMH_PACKED_LPR: 4 | 16 lanes per packed row; 0 = by the row width
  std::atomic<long long> packed_unroll{0};       // FMH_PACKED_UNROLL: batch depth of the packed cores; 0 = fewest padded slots
  std::atomic<long long> packed_no_prefetch{0};  // FMH_PACKED_NO_PREFETCH: plain row loop instead of tile_rows_packed_prefetch
  std::atomic<long long> counts_mfma{0};         // FMH_COUNTS_MFMA: 1 | 2 = the int8 matrix-core counting route (BASELINE config C5)
  std::atomic<long long> grid_per_cu{0};         // FMH_GRID_PER_CU: workgroups per CU of the persistent grid; 0 = the occupancy
  std::atomic<long long> grid_blocks{0};         // FMH_GRID_BLOCKS: total workgroups (tests: many tile rounds on small inputs)
  std::atomic<long long> max_occ{0};             // FMH_MAX_OCC: cap on the occupancy used for the grid
  std::atomic<long long> unroll{0};              // FMH_UNROLL: 8 = deeper batches of the u8 cores
  std::atomic<long long> pitch_align{16};        // FMH_PITCH_ALIGN: row pitch alignment of u8 matrices
  std::atomic<long long> comm_host{0};           // FMH_COMM_TRANSPORT = host: in-process rendezvous instead of RCCL (fmh_comm_init_all)
  std::atomic<long long> upload_threads{0};      // FMH_UPLOAD_THREADS: host packer threads; 0 = the CPU share
  std::atomic<long long> pd_two_planes{0}, pd_int8{0}, pd_planes_bytes{(long long)8 << 30}, pd_kchunk{0}, pd_sb{0}, pd_occ{0}, pd_phased{1}, pd_slabs{1}, pd_slab_bytes{(long long)4 << 30};  // FMH_PD_*: pairwise path
  std::atomic<long long> pipe{-1};               // FMH_PIPE: the pipelined tile loop on four-lane rows: 1 = wherever it is built, 0 = never, -1 = where it measured ahead (one and two groups)
  std::atomic<long long> flat{-1};               // FMH_FLAT: the LDS-staged flat-tile route on short packed rows: 1 = wherever it is built, 0 = never, -1 = where it measured ahead
  std::atomic<long long> flat_slots{0};          // FMH_FLAT_SLOTS: 0 = the register-staged variant (default); 1 | 2 = the LDS-DMA variants with that many tile images per wave
  std::atomic<long long> flat_defer{0};          // FMH_FLAT_DEFER: tiles a wave counts before it runs their epilogues on the register-staged variant (1..8); 0 = by the launch size
  std::atomic<long long> wc_exact{1};            // FMH_WC_EXACT: 0 = five to seven W&C groups run the padded eight-group kernel again (A/B of the exact kernels)
  std::atomic<long long> wc_bi_totals{1};        // FMH_WC_BI_TOTALS: 0 = more than eight groups' regional sums through the general pair kernel again (A/B of the biallelic one)
  std::atomic<long long> wc_bi_replicas{0};      // FMH_WC_BI_REPLICAS: 1 | 2 | 4 | 8 threads per pair in the biallelic pair kernel; 0 = by the lanes the last wave would waste
  std::atomic<long long> wc_bi_chunks{0};        // FMH_WC_BI_CHUNKS: row chunks of the biallelic pair kernel (measurement); 0 = about 8 192 workgroups
  std::atomic<long long> row_hi{1};              // FMH_ROW_HI: 0 = packed matrices get no tables of the rows with alleles above 1 / with uncalled columns (every plane of every row is read); 2 = tables at any size
  std::atomic<long long> column_window{1};       // FMH_COLUMN_WINDOW: 0 = every sweep reads every vector of a row and no row totals are kept; 1 = sweeps read the vectors their groups have members in, row totals for packed biallelic matrices of >= 4 096 rows with nothing missing; 2 = row totals at any size
  std::atomic<long long> tiled_planes{1};        // FMH_TILED_PLANES: the tile-transposed image of plane 0 (fmh_matrix::p0t): 0 = never built; 1 (default) = packed biallelic matrices of >= 4 096 rows with nothing missing, while the image fits under FMH_TILED_BYTES and as much again stays free; 2 = at any size, no free-memory test
  std::atomic<long long> tiled_bytes{(long long)16 << 30};  // FMH_TILED_BYTES: the largest image FMH_TILED_PLANES=1 builds
  std::atomic<long long> tiled{-1};              // FMH_TILED: 0 = sweeps take the row-major routes even where the image exists (the A side of every A/B); 1 = the tiled route wherever it is built; -1 = where it measured ahead (tiled_route_default)
  std::atomic<long long> prefix_counts{1};       // FMH_PREFIX_COUNTS: the per-row prefix counts of plane 0 at every vector boundary (fmh_matrix::p0c): 0 = never built, never read; 1 (default) = beside the image, on matrices of >= 4 096 rows and at most 65 535 columns while as much again stays free; 2 = beside the image at any size, no free-memory test
  std::atomic<long long> tiled_batch{0};         // FMH_TILED_BATCH = 10 | 5 | 2: the half batch of the tiled sweep (measurements); 0 = by the window (sweep_tiled.hip)
  std::atomic<long long> pca_eigen{0};           // FMH_PCA_EIGEN = host | rocsolver: the PCA's symmetric eigen solver; 0 = rocSOLVER, the host solver when it cannot be loaded
  std::atomic<long long> pca_splits{0};          // FMH_PCA_SPLITS: K splits of the PCA Gram (1 = none); 0 = by the tile count
  std::atomic<long long> pca_budget_bytes{(long long)16 << 30};  // FMH_PCA_BUDGET_BYTES: device memory one fmh_pca_gram call may use (Gram + bit words + slabs)
  std::atomic<long long> grm_splits{0};          // FMH_GRM_SPLITS: K splits of the relationship matrix's Gram (1 = none); 0 = by the tile count
  std::atomic<long long> sfs_item_rows{0};       // FMH_SFS_ITEM_ROWS: rows per work item of the site frequency spectrum kernel; 0 = 4 096
  std::atomic<long long> sfs_lds_bins{0};        // FMH_SFS_LDS_BINS: cap on that kernel's LDS tile in bins (tests: tiny shapes take the global path and the corner mapping); 0 = 5 116, an eighth of a CU's LDS (at most 40 956, all of it)
  std::atomic<long long> hap_threads{0};         // FMH_HAP_THREADS = 64 | 256 | 512 | 1024: threads per workgroup of the haplotype window kernel (raised where a group needs more); 0 = by the group size
  std::atomic<long long> fstat_item_rows{0};     // FMH_FSTAT_ITEM_ROWS: rows per work item of the f-statistics moment kernel; 0 = 4 096
  std::atomic<long long> fstat_lds_mask_bytes{0};  // FMH_FSTAT_LDS_MASK_BYTES: LDS bytes that kernel's mask entries may take; 0 = 8 192 (eight workgroups per CU stay resident); entries that need more are read from global memory (1 forces that)
  std::atomic<long long> kin_budget_bytes{(long long)16 << 30};  // FMH_KIN_BUDGET_BYTES: the Gram scratch one fmh_kinship_counts call may take
  std::atomic<long long> qc_item_rows{0};        // FMH_QC_ITEM_ROWS: rows per work item of the genotype QC kernels; 0 = 4 096
  std::atomic<long long> lmm_item_rows{0};       // FMH_LMM_ITEM_ROWS: the most rows per work item of the mixed-model projections; 0 = 4 096, fewer on short ranges
  std::atomic<long long> admix_item_rows{0};     // FMH_ADMIX_ITEM_ROWS: usable rows per work item of the admixture step, rounded up to whole passes of 128; 0 = two items per compute unit, fewer where the slabs would pass the budget
  std::atomic<long long> admix_budget_bytes{(long long)4 << 30};  // FMH_ADMIX_BUDGET_BYTES: device bytes the code image of an fmh_admix handle plus the padded state and slabs of one fmh_admix_step may take
  std::atomic<long long> assoc_item_rows{0};     // FMH_ASSOC_ITEM_ROWS: rows per work item of the association scans' sums kernels; 0 = 4 096 (DESIGN.md sections 3.18, 3.19)
  std::atomic<long long> assoc_budget_bytes{(long long)1 << 30};  // FMH_ASSOC_BUDGET_BYTES: device bytes the sums of one row chunk of ferromic.association_scan / logistic_scan may take
  std::atomic<long long> score_item_rows{0};     // FMH_SCORE_ITEM_ROWS: rows per work item of the polygenic score's sums kernel, rounded up to a multiple of 64; 0 = 4 096
  std::atomic<long long> score_budget_bytes{(long long)1 << 30};  // FMH_SCORE_BUDGET_BYTES: device bytes the digits and slabs of one fmh_score_sums call may take; ferromic.polygenic_score sizes its row chunks by it
  std::atomic<long long> roh_item_rows{0};       // FMH_ROH_ITEM_ROWS: kept rows per work item of the runs-of-homozygosity scan kernel, rounded up to a multiple of 64; 0 = 4 096
  std::atomic<long long> ibd_item_rows{0};       // FMH_IBD_ITEM_ROWS: kept rows per row block of the IBD pair kernel, rounded up to a multiple of 64; 0 = sized by the launch
  std::atomic<long long> ibd_budget_bytes{(long long)4 << 30};  // FMH_IBD_BUDGET_BYTES: device bytes the sample-major bit image and the block records of one fmh_ibd_scan call may take
  std::atomic<long long> clump_budget_bytes{(long long)1 << 30};  // FMH_CLUMP_BUDGET_BYTES: device bytes of threshold words one launch of fmh_clump's tile kernel may write; candidates are walked in chunks under it
  std::atomic<long long> clump_host_bytes{(long long)8 << 30};    // FMH_CLUMP_HOST_BYTES: host bytes of all candidates' threshold bit rows, kept for fmh_clump's greedy pass; more is refused
  std::atomic<long long> ldscore_budget_bytes{(long long)1 << 30};  // FMH_LDSCORE_BUDGET_BYTES: device scratch of one launch of fmh_ld_scores (28 bytes per kept row + 8 per item); the items are walked in chunks under it
  std::atomic<long long> graph{0};               // FMH_GRAPH: 1 = replay a repeated pipelined sweep on a local communicator from a captured hipGraph
  std::atomic<unsigned long long> generation{0}; // bumped by every fmh_set_option: a captured launch is never replayed across an option change
};
Options& options();

// FMH_LAYOUT=bytes keeps the u8 kernels on matrices that still hold their byte rows
inline bool layout_bytes_forced() { return options().layout_bytes.load(std::memory_order_relaxed) != 0; }

// RAII for the scratch of one call
struct DeviceScratch {
  int device = 0;
  hipStream_t stream = nullptr;
  bool settled = false;  // set once the call has synchronised the stream its kernels ran on
  std::vector<void*> ptrs;
  DeviceScratch() = default;
  DeviceScratch(int device_, hipStream_t stream_) : device(device_), stream(stream_) {}
  // An early (error) return may leave kernels that write these blocks enqueued: wait for the stream before the blocks go
  // back to the pool, where another thread's pool_malloc could be handed them at once.
  ~DeviceScratch() {
    if (!settled && !ptrs.empty()) { (void)hipStreamSynchronize(stream); (void)hipGetLastError(); }
    for (void* p : ptrs) pool_free(device, p);
  }
  template <class T> int get(T** out, size_t count) {
    void* p = nullptr;
    HIP_TRY(pool_malloc(device, &p, (count > 0 ? count : 1) * sizeof(T)));
    ptrs.push_back(p);
    *out = (T*)p;
    return FMH_OK;
  }
};

// ---- per-device workspace: sweep leases, harmonic table, pairwise scratch -----------------------------------------------
// What ONE sweep in flight needs: block partials, the finalised totals, their pinned host copy, timing events, and a stream of its own
// (used when the caller passes the NULL stream, so that sweeps issued by different host threads overlap on the device instead of
// queueing behind each other on the legacy default stream).  Leases are pooled per device: run_vcf's region workers each take one.
struct SweepLease {
  double* part_f64 = nullptr;
  unsigned long long* part_u64 = nullptr;
  double* out_f64 = nullptr;
  unsigned long long* out_u64 = nullptr;
  double* h_f64 = nullptr;  // pinned
  unsigned long long* h_u64 = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t stream = nullptr;
};
struct Workspace {
  bool ready = false;
  int cus = 0;
  int max_grid = 0;
  std::mutex lease_mu;
  std::vector<SweepLease*> idle_leases;
  double* harmonic = nullptr;  // grows only; superseded tables stay alive (a sweep in flight may still read them)
  size_t harmonic_len = 0;
  std::vector<double*> retired_harmonic;
  uint8_t* pd_planes = nullptr;  // pairwise-differences planes, kept between calls (fmh_device_release_scratch frees them)
  size_t pd_planes_bytes = 0;
  int* pd_slabs = nullptr;       // the phased Gram kernel's per-item partial tiles
  size_t pd_slab_bytes = 0;
  std::mutex in_use;  // the harmonic table's growth and the pairwise scratch: one holder at a time per device
};
int workspace(int device, Workspace** out);
// the device's two LDS figures (abi.hip, filled by workspace()): what a workgroup's masks may take, and the LDS of a CU
size_t device_lds_limit(int device);
size_t device_lds_per_cu(int device);
// one sweep's buffers, taken from / returned to the device's pool; the device's harmonic table grown to index max_k (abi.hip)
int lease_acquire(Workspace* w, SweepLease** out);
struct LeaseHolder {
  Workspace* w = nullptr;
  SweepLease* l = nullptr;
  ~LeaseHolder() {
    if (w && l) { std::lock_guard<std::mutex> lock(w->lease_mu); w->idle_leases.push_back(l); }
  }
};
int ensure_harmonic(Workspace* w, size_t max_k, hipStream_t st);

// measurement (fmh_timing_*): accumulated HIP-event time of the sweep kernels
void timing_add(double ms);
bool timing_enabled();

// ---- kernel launches that live in their own translation units ------------------------------------------------------
// What a launcher needs from the workspace.
struct LaunchCtx {
  int cus;
  int max_grid;
  hipEvent_t ev0, ev1;  // recorded around the sweep kernel when `timing`
  bool timing;
};
// Device buffers a sweep reduces into: [grid][64] block partials and the 64 + 64 regional accumulators.
struct SweepBuffers {
  double* part_f64;
  unsigned long long* part_u64;
  double* out_f64;
  unsigned long long* out_u64;
  // optional: run finalize_kernel on another stream, ordered behind the sweep by this event - the pipelined sharded sweeps put it on the
  // communicator's stream, so that the next window's sweep follows this one's without the finalize launch and its two kernel boundaries between them
  hipStream_t finalize_stream = nullptr;
  hipEvent_t swept = nullptr;
};
}  // namespace fmhi
struct fmh_matrix;
struct fmh_groups;
namespace fmhi {
// host buffers -> the (already allocated) planes of a packed matrix (upload.hip): packed on the host into pinned staging, copied
// asynchronously; *overflow = a called entry carries an allele above max_allele
int upload_planes_from_bytes(fmh_matrix* m, const uint8_t* h_data, const uint64_t* h_missing, bool* overflow);
int upload_planes_from_planes(fmh_matrix* m, const uint8_t* const h_planes[4], size_t h_pitch);
void upload_release(int device);
// planes rows [row0, row0 + rows) of a packed matrix -> byte rows of `pitch` bytes (abi.hip)
hipError_t unpack_rows(const fmh_matrix* m, size_t row0, size_t rows, uint8_t* data, size_t pitch, hipStream_t st);
// sweep + finalize enqueued on `st`, no synchronisation (sweep_dispatch.hip)
int enqueue_sweep(const fmh_matrix* m, const fmh_groups* g, int mode, fmh::SweepArgs& a, hipStream_t st, const LaunchCtx& ctx,
                  const SweepBuffers& b, const double* harmonic, bool* launched);
// the blocking form the statistic entry points use: a lease of the device's workspace, enqueue_sweep, synchronise, the totals on the host
struct SweepResult {
  double f64[fmh::kMaxF64];
  unsigned long long u64[fmh::kMaxU64];
};
int run_sweep(const fmh_matrix* m, const fmh_groups* g, int mode, fmh::SweepArgs& a, void* stream, SweepResult* res);
int launch_finalize(const double* part_f64, const unsigned long long* part_u64, int grid, double* out_f64, unsigned long long* out_u64, hipStream_t st);  // abi.hip

// What a sweep of `mode` over these groups reads of every row (sweep_plan.hpp): vectors [first, first + count) of plane 0, and the
// group whose alt count comes from the matrix's row totals instead of being counted (-1: none).  The whole row and -1 unless the image is
// packed, biallelic and has nothing missing.
struct ColumnWindow {
  uint32_t first, count;
  int derived;
};
ColumnWindow sweep_window(const fmh_matrix* m, const fmh_groups* g, int mode);

// the fused region sweep's kernel arguments and mode (abi.hip); the device's harmonic table
int pair_region_args(const fmh_groups* g, size_t row_begin, size_t row_count, int summary_formula, int hudson_formula, const fmh_pair_diversity_sites* div,
                     const fmh_hudson_sites* sites, fmh::SweepArgs& a, int* mode);
int harmonic_table(int device, size_t max_k, hipStream_t st, const double** out);
// W&C slot order of the padded kernel -> the caller's pair order (abi.hip); the kernel's group count and which W&C / summaries calls
// are one fused sweep (sweep_dispatch.hip, from the predicates of sweep_plan.hpp)
void wc_slot_map(const fmh_matrix* m, const fmh_groups* g, fmh::SweepArgs& a);
int wc_kernel_groups(const fmh_matrix* m, const fmh_groups* g);
bool wc_fused_lane_totals(const fmh_matrix* m, const fmh_groups* g);
bool summaries_single_sweep(const fmh_matrix* m, const fmh_groups* g);

// the pieces of fmh_pca_gram_sharded that live beside the Gram (pca.hip): every check of fmh_pca_gram plus `extra_bytes` against the budget,
// nothing allocated or enqueued (n_kept == 0 is valid here); the upper triangle of an n x n matrix packed / unpacked with the mirror on `st`
int pca_gram_check(const fmh_matrix* m, const uint64_t* h_kept_rows, size_t n_kept, const double* h_set_value, const double* h_clear_value,
                   double* d_gram, size_t extra_bytes);
int pca_pack_triangle(const double* d_full, size_t n, double* d_tri, hipStream_t st);
int pca_unpack_triangle(const double* d_tri, size_t n, double* d_full, hipStream_t st);
// the top eigenpairs of a symmetric device matrix (overwritten) through the solver FMH_PCA_EIGEN names (pca.hip): lambda[k] descending,
// row k of `top` the unit eigenvector; arguments already checked
int pca_eigen_top(int device, double* d_matrix, size_t n, size_t n_components, std::vector<double>& lambda, std::vector<double>& top);

// One function per (mask route, lanes per row): dispatches on (P, mode, missing, general) to the instantiation, sizes the
// persistent grid and launches.  FMH_ERR_UNSUPPORTED for a combination the route does not build.
int launch_sweep_packed4(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
int launch_sweep_packed16(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
// three-plane packed matrices (alleles 4..7): the multi-allelic kernels only
int launch_sweep_packed4_3p(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
int launch_sweep_packed16_3p(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
int launch_sweep_bytes(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
int launch_sweep_bits(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
int launch_sweep_global(int P, int mode, bool missing, bool general, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);
// the LDS-staged flat-tile route (sweep_flat.hip): packed rows of at most kFlatMaskMaxVec vectors, biallelic, nothing missing
constexpr int kFlatMaskMaxVec = 32;
// The (P, mode) pairs each of the three routes is built for, ONE list per route: *_route_builds (what the plan asks) and the route's
// dispatcher (what is instantiated) are both written from it.
#define FMH_FLAT_BUILDS(X)                                                                                                         \
  X(1, fmh::kModeSummary) X(2, fmh::kModeSummary) X(4, fmh::kModeSummary) X(2, fmh::kModeSummary | fmh::kModeHudson)                  \
  X(1, fmh::kModeSummary | fmh::kModeDiversity) X(2, fmh::kModeSummary | fmh::kModeDiversity)                                        \
  X(2, fmh::kModeSummary | fmh::kModeHudson | fmh::kModeDiversity) X(2, fmh::kModeWc) X(4, fmh::kModeWc)
#define FMH_TILED_BUILDS(X)                                                                                                        \
  X(1, fmh::kModeSummary) X(2, fmh::kModeSummary) X(2, fmh::kModeSummary | fmh::kModeHudson)                                         \
  X(1, fmh::kModeSummary | fmh::kModeDiversity) X(2, fmh::kModeSummary | fmh::kModeDiversity)                                        \
  X(2, fmh::kModeSummary | fmh::kModeHudson | fmh::kModeDiversity)
#define FMH_MFMA_BUILDS(X)                                                                                                         \
  X(1, fmh::kModeSummary) X(2, fmh::kModeSummary) X(4, fmh::kModeSummary) X(2, fmh::kModeSummary | fmh::kModeHudson)                  \
  X(1, fmh::kModeSummary | fmh::kModeDiversity) X(2, fmh::kModeWc) X(4, fmh::kModeWc)
#define FMH_ROUTE_BUILDS_ROW(PV, MODEV) if (P == PV && mode == (MODEV)) return true;
inline bool flat_route_builds(int P, int mode) { FMH_FLAT_BUILDS(FMH_ROUTE_BUILDS_ROW) return false; }
inline bool flat_route_default(int P, int mode, uint32_t pvec) { (void)P; (void)mode; (void)pvec; return false; }  // until measured
int launch_sweep_flat(int P, int mode, const fmh::SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid);
// the sweep over the tile-transposed image of plane 0 (sweep_tiled.hip): packed, biallelic, nothing missing, one or two groups, not W&C
inline bool tiled_route_builds(int P, int mode) { FMH_TILED_BUILDS(FMH_ROUTE_BUILDS_ROW) return false; }
// The default rule (FMH_TILED=-1), by measurement (profiles/tiled_planes/): at equal bytes the tiled kernel is about 7 % behind
// the four-lane ones (the whole row at 5 000 haplotypes), so it is taken where it reads clearly fewer: a window of at most seven eighths of the row.
// Measured ahead at 20 and 9 of 40 vectors with a group derived (1.11-1.65x), 27 of 40 without (1.28-1.36x), 10 of 20 and 4 of 8 (1.08-1.58x);
// measured behind at 39 and 40 of 40 (3-9 % at 2.5 M sites and more), which therefore keep the row-major routes.
inline bool tiled_route_default(uint32_t window_vecs, uint32_t pvec) { return (uint64_t)window_vecs * 8 <= (uint64_t)pvec * 7; }
int launch_sweep_tiled(int P, int mode, const fmh::SweepArgs& a, hipStream_t st, const LaunchCtx& ctx, int* grid);
// counts on the int8 matrix cores (sweep_mfma.hip): u8 rows, biallelic, nothing missing, at most 4 (padded) groups
int launch_sweep_mfma(int P, int mode, const fmh::SweepArgs& a, size_t smem, hipStream_t st, const LaunchCtx& ctx, int* grid);

}  // namespace fmhi

// ---- handles (the opaque types of the C-ABI) ----------------------------------------------------------------------------
struct fmh_matrix {
  int device = 0;
  uint8_t* data = nullptr;
  uint8_t* bits = nullptr;  // called bit-rows or null
  size_t pitch = 0, bits_pitch = 0;
  size_t variants = 0, samples = 0, ploidy = 0;
  uint32_t columns = 0, nvec = 0;
  uint8_t max_allele = 0;
  bool owns = true;
  bool has_missing = false;  // a called mask exists (bits and / or pc)
  // bit-packed image (fmh_matrix_pack): plane k = bit k of the allele value (p1: max_allele >= 2, p2: max_allele >= 4),
  // pc = called bits; plane_pitch bytes per row, pvec = ceil(columns / 128) 16-byte vectors.  data / bits may have been
  // released (nullptr).
  uint8_t *p0 = nullptr, *p1 = nullptr, *p2 = nullptr, *pc = nullptr;
  uint8_t* row_gap = nullptr; // with pc: one byte per row, non-zero when some column of the row is not called (written wherever the planes are)
  uint32_t* row_alt = nullptr;  // biallelic with nothing missing: popcount of plane 0 over the row's columns (rebuilt or dropped wherever the planes are written)
  // plane 0 tile-transposed: the 16 bytes of row r, vector v at byte (((r >> 6) * pvec + v) * 64 + (r & 63)) * 16, rows past
  // `variants` in the last tile zero; biallelic with nothing missing only.  It DOUBLES the resident planes (6.4 GB at 10 M x 5 000); rebuilt or dropped
  // wherever row_alt is.  A column window of a sweep is then whole KiB of every tile: no fetched line holds a byte the sweep does not need.
  uint8_t* p0t = nullptr;
  size_t p0t_bytes = 0;
  // prefix counts of plane 0: for image tile T, boundary b in [0, pvec] and row slot s, the u16 at byte
  // ((T * (pvec + 1) + b) * 64 + s) * 2 is the popcount of that row over vectors [0, b) - one 128-byte line per boundary and tile; b = pvec equals
  // row_alt.  Only beside p0t and on rows of at most 65 535 columns; rebuilt or dropped wherever p0t is.
  uint16_t* p0c = nullptr;
  size_t p0c_bytes = 0;
  uint8_t* row_hi = nullptr;  // with p1: one byte per row, non-zero when the row has a bit in plane 1 or 2 (written wherever the planes are)
  size_t plane_pitch = 0;
  uint32_t pvec = 0;
};

struct fmh_groups {
  int device = 0;
  int n_groups = 0;   // caller's P
  int padded = 0;     // kernel P (1, 2, 4 or 8)
  uint8_t* masks = nullptr;  // [padded][mask_pitch], zero beyond the row
  size_t pitch = 0;
  size_t mask_pitch = 0;     // pitch rounded up to 2048: covers the kernels' zero-padded mask stride
  uint16_t* mask_bits = nullptr;  // [padded][mask_pitch / 16]: the same masks as one 16-bit word per 16-byte vector
  uint32_t* mask_flat = nullptr;  // [round_up(ceil(columns / 128), 4)][padded][4]: the bit masks interleaved by vector (rows of at most 4 096 columns; same block)
  uint32_t columns = 0;
  uint64_t sizes[FMH_MAX_GROUPS] = {0};
  // column geometry (fmh_groups_create): the first and last 128-column vector each group has a member in (first > last: no member), and whether
  // the groups are pairwise disjoint / cover every column - together: a partition, the case in which one group's counts follow from the row totals
  uint32_t vec_first[FMH_MAX_GROUPS] = {0}, vec_last[FMH_MAX_GROUPS] = {0};
  bool disjoint = false, covers = false;
  // contiguous[p]: the members of group p are exactly the columns [col_first[p], col_end[p]), at least one of them
  uint32_t col_first[FMH_MAX_GROUPS] = {0}, col_end[FMH_MAX_GROUPS] = {0};
  bool contiguous[FMH_MAX_GROUPS] = {false};
  std::vector<uint8_t> host_mask;  // [n_groups][columns] as handed in (the wide-matrix W&C route re-batches the groups)
};
