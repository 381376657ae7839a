// pca.hip — the haplotype PCA of src/pca.rs on the device: fmh_pca_scan_sites (the inputs of the site filter), fmh_pca_gram
// (gather + transpose of the kept sites, the f64 matrix-core Gram of the standardised matrix) and fmh_pca_eigen_scores (the n x n
// symmetric eigenproblem through rocSOLVER, bound at run time, or a plain host solver; scores = U sqrt((n - 1) lambda)).
// Kernels in pca_kernels.hpp.  The filter decision and the standardisation constants stay with the caller, in f64 on the host,
// so that they are the reference's arithmetic.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "abi_internal.hpp"
#include "pca_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

// efficient_pca::pca::NEAR_ZERO_THRESHOLD (pca.rs:2).  UNVERIFIED: the crate's source was not available when this was written; the
// value only decides whether a numerically-zero eigenvalue yields a zero column, and no test depends on it.
constexpr double kNearZeroThreshold = FMH_PCA_NEAR_ZERO_THRESHOLD;

bool use_packed(const fmh_matrix* m) { return m->p0 && !(m->data && layout_bytes_forced()); }

// ---- rocSOLVER, bound at run time (types as in <rocblas/rocblas.h> / <rocsolver/rocsolver.h>) ------------------------------------------
typedef struct _rocblas_handle* rocblas_handle;
typedef int rocblas_status;  // rocblas_status_success == 0
typedef int32_t rocblas_int;
constexpr int kEvectOriginal = 211;  // rocblas_evect_original
constexpr int kFillLower = 122;      // rocblas_fill_lower

struct SolverApi {
  void* lib = nullptr;
  std::string origin;
  rocblas_status (*create_handle)(rocblas_handle*) = nullptr;
  rocblas_status (*set_stream)(rocblas_handle, hipStream_t) = nullptr;
  rocblas_status (*dsyevd)(rocblas_handle, int, int, rocblas_int, double*, rocblas_int, double*, double*, rocblas_int*) = nullptr;
  std::map<int, rocblas_handle> handles;  // one per device, kept for the life of the process
};
SolverApi g_solver;
std::mutex g_solver_mutex;
// a rocBLAS handle is not thread-safe: one eigenproblem at a time per device (two host threads may call with the GIL released)
std::mutex g_solver_device_mutex[64];

int solver_api(int device, SolverApi** out, rocblas_handle* handle) {
  std::lock_guard<std::mutex> lock(g_solver_mutex);
  if (!g_solver.lib) {
    void* h = nullptr;
    std::string origin;
    // (1) a copy this process already maps, (2) an explicit path, (3) the system's
    for (const char* name : {"librocsolver.so", "librocsolver.so.0"}) {
      if (!h && (h = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) origin = std::string(name) + " (already loaded)";
    }
    if (!h) {
      if (const char* env = getenv("FMH_ROCSOLVER_LIBRARY")) { if ((h = dlopen(env, RTLD_NOW | RTLD_LOCAL))) origin = env; }
    }
    // the copy that sits next to the HIP runtime this process runs on (a PyTorch wheel bundles both) before the system's
    Dl_info rt;
    if (!h && dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &rt) && rt.dli_fname) {
      std::string dir(rt.dli_fname);
      const size_t slash = dir.rfind('/');
      if (slash != std::string::npos) {
        dir.resize(slash + 1);
        for (const char* name : {"librocsolver.so.0", "librocsolver.so"}) {
          if (!h && (h = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL))) origin = dir + name;
        }
      }
    }
    for (const char* name : {"librocsolver.so.0", "librocsolver.so", "/opt/rocm/lib/librocsolver.so.0", "/opt/rocm/lib/librocsolver.so"}) {
      if (!h && (h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) origin = name;
    }
    if (!h) return fail(FMH_ERR_UNSUPPORTED, "rocSOLVER is not available (dlopen librocsolver.so: %s); set FMH_ROCSOLVER_LIBRARY or FMH_PCA_EIGEN=host", dlerror());
    SolverApi api;
    api.lib = h;
    api.origin = origin;
#define BIND(field, sym)                                                   \
  api.field = reinterpret_cast<decltype(api.field)>(dlsym(h, sym));        \
  if (!api.field) return fail(FMH_ERR_UNSUPPORTED, "rocSOLVER (%s) lacks %s", origin.c_str(), sym)
    BIND(create_handle, "rocblas_create_handle");  // rocBLAS is a dependency of rocSOLVER: dlsym searches it too
    BIND(set_stream, "rocblas_set_stream");
    BIND(dsyevd, "rocsolver_dsyevd");
#undef BIND
    g_solver = api;
  }
  auto it = g_solver.handles.find(device);
  if (it == g_solver.handles.end()) {
    rocblas_handle hd = nullptr;
    if (g_solver.create_handle(&hd) != 0 || !hd) return fail(FMH_ERR_HIP, "rocblas_create_handle failed on device %d", device);
    it = g_solver.handles.emplace(device, hd).first;
  }
  *out = &g_solver;
  *handle = it->second;
  return FMH_OK;
}

// ---- host solver: Householder tridiagonalisation + implicit QL (the EISPACK tred2 / tql2 pair) -------------------------------------
// a: n x n symmetric, row-major; on return column k of `a` is the unit eigenvector of w[k], w ascending.
void eigen_symmetric_host(double* a, size_t n_, double* w) {
  const long n = (long)n_;
  std::vector<double> ev((size_t)n, 0.0);
  double* d = w;
  double* e = ev.data();
  auto V = [&](long i, long j) -> double& { return a[(size_t)i * n + j]; };
  for (long j = 0; j < n; ++j) d[j] = V(n - 1, j);
  for (long i = n - 1; i > 0; --i) {
    double scale = 0.0, h = 0.0;
    for (long k = 0; k < i; ++k) scale += std::fabs(d[k]);
    if (scale == 0.0) {
      e[i] = d[i - 1];
      for (long j = 0; j < i; ++j) { d[j] = V(i - 1, j); V(i, j) = 0.0; V(j, i) = 0.0; }
    } else {
      for (long k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
      double f = d[i - 1], g = std::sqrt(h);
      if (f > 0) g = -g;
      e[i] = scale * g;
      h -= f * g;
      d[i - 1] = f - g;
      for (long j = 0; j < i; ++j) e[j] = 0.0;
      for (long j = 0; j < i; ++j) {
        f = d[j];
        V(j, i) = f;
        g = e[j] + V(j, j) * f;
        for (long k = j + 1; k <= i - 1; ++k) { g += V(k, j) * d[k]; e[k] += V(k, j) * f; }
        e[j] = g;
      }
      f = 0.0;
      for (long j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
      const double hh = f / (h + h);
      for (long j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (long j = 0; j < i; ++j) {
        f = d[j];
        g = e[j];
        for (long k = j; k <= i - 1; ++k) V(k, j) -= f * e[k] + g * d[k];
        d[j] = V(i - 1, j);
        V(i, j) = 0.0;
      }
    }
    d[i] = h;
  }
  for (long i = 0; i < n - 1; ++i) {  // accumulate the transformations
    V(n - 1, i) = V(i, i);
    V(i, i) = 1.0;
    const double h = d[i + 1];
    if (h != 0.0) {
      for (long k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
      for (long j = 0; j <= i; ++j) {
        double g = 0.0;
        for (long k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
        for (long k = 0; k <= i; ++k) V(k, j) -= g * d[k];
      }
    }
    for (long k = 0; k <= i; ++k) V(k, i + 1) = 0.0;
  }
  for (long j = 0; j < n; ++j) { d[j] = V(n - 1, j); V(n - 1, j) = 0.0; }
  V(n - 1, n - 1) = 1.0;
  e[0] = 0.0;
  // implicit QL on the tridiagonal (d, e); the rotations run over the TRANSPOSE so that a vector is a contiguous row
  auto transpose = [&] { for (long i = 0; i < n; ++i) for (long j = i + 1; j < n; ++j) std::swap(V(i, j), V(j, i)); };
  transpose();
  for (long i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  double f = 0.0, tst1 = 0.0;
  const double eps = std::ldexp(1.0, -52);
  for (long l = 0; l < n; ++l) {
    tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
    long m = l;
    while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;
    if (m > l) {
      do {
        double g = d[l];
        double p = (d[l + 1] - g) / (2.0 * e[l]);
        double r = std::hypot(p, 1.0);
        if (p < 0) r = -r;
        d[l] = e[l] / (p + r);
        d[l + 1] = e[l] * (p + r);
        const double dl1 = d[l + 1];
        double h = g - d[l];
        for (long i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
        const double el1 = e[l + 1];
        for (long i = m - 1; i >= l; --i) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = std::hypot(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          double* vi = a + (size_t)i * n;
          double* vi1 = vi + n;
          for (long k = 0; k < n; ++k) {
            h = vi1[k];
            vi1[k] = s * vi[k] + c * h;
            vi[k] = c * vi[k] - s * h;
          }
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
      } while (std::fabs(e[l]) > eps * tst1);
    }
    d[l] += f;
    e[l] = 0.0;
  }
  for (long i = 0; i < n - 1; ++i) {  // ascending
    long k = i;
    for (long j = i + 1; j < n; ++j) if (d[j] < d[k]) k = j;
    if (k != i) {
      std::swap(d[k], d[i]);
      std::swap_ranges(a + (size_t)i * n, a + (size_t)(i + 1) * n, a + (size_t)k * n);
    }
  }
  transpose();
}

// stage times of the calling thread's last fmh_pca_gram that ran with fmh_timing_enable on: transpose, Gram, slab reduce (ms)
// [3] site scan (events, the last timed fmh_pca_scan_sites), [4] the eigen solver of the last fmh_pca_eigen_scores (events around
// rocsolver_dsyevd, or the host solver's wall clock), [5] which solver that was: 1 = host, 2 = rocSOLVER
thread_local double g_pca_stage_ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

}  // namespace

extern "C" int fmh_timing_read_pca(double* h_stage_ms) {
  if (!h_stage_ms) return fail(FMH_ERR_INVALID, "h_stage_ms is NULL");
  for (int i = 0; i < 6; ++i) h_stage_ms[i] = g_pca_stage_ms[i];
  return FMH_OK;
}

extern "C" int fmh_pca_eigen_host(double* h_matrix, size_t n, double* h_eigenvalues) {
  if (!h_matrix || !h_eigenvalues) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n == 0) return fail(FMH_ERR_INVALID, "n is 0");
  eigen_symmetric_host(h_matrix, n, h_eigenvalues);
  return FMH_OK;
}

extern "C" int fmh_pca_scan_sites(const fmh_matrix* m, size_t row_begin, size_t row_count, uint32_t* d_alt_count, uint8_t* d_flags, void* stream) {
  if (!m || !d_alt_count || !d_flags) return fail(FMH_ERR_INVALID, "NULL argument");
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  FMH_TRY(use_device(m->device));
  if (row_count == 0) return FMH_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((row_count + 3) / 4));
  KernelTimer<> timer;
  FMH_TRY(timer.start(st));
  if (use_packed(m)) {
    hipLaunchKernelGGL(pca_scan_packed_kernel, grid, dim3(256), 0, st, m->p0, m->p1, m->p2, m->pc, m->pc ? m->row_gap : nullptr,
                       (m->p1 || m->p2) ? m->row_hi : nullptr, m->plane_pitch, m->columns, row_begin, row_count, d_alt_count, d_flags);
  } else {
    if (!m->data) return fail(FMH_ERR_INVALID, "the matrix holds neither a packed image nor byte rows");
    hipLaunchKernelGGL(pca_scan_bytes_kernel, grid, dim3(256), 0, st, m->data, m->pitch, m->bits, m->bits_pitch, m->columns, row_begin, row_count,
                       d_alt_count, d_flags);
  }
  HIP_TRY(hipGetLastError());
  FMH_TRY(timer.stop(st));
  HIP_TRY(hipStreamSynchronize(st));
  return timer.elapsed(0, &g_pca_stage_ms[3]);
}

namespace {
// fmh_pca_gram; `extra_bytes` = device memory the caller needs beside it (counted against the budget), `check_only` = return once every
// argument and the budget have been checked, before anything is allocated or enqueued
int gram_impl(const fmh_matrix* m, const uint64_t* h_kept_rows, size_t n_kept, const double* h_set_value, const double* h_clear_value, double* d_gram,
              void* stream, size_t extra_bytes, bool check_only) {
  if (!m || !d_gram) return fail(FMH_ERR_INVALID, "NULL argument");
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "haplotype PCA needs diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  const size_t n = m->samples * 2;
  if (n < 2) return fail(FMH_ERR_INVALID, "haplotype PCA needs at least two haplotypes");
  if (n_kept == 0) return fail(FMH_ERR_INVALID, "no kept sites (n_kept is 0)");
  if (!h_kept_rows || !h_set_value || !h_clear_value) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n > ((size_t)1 << 24) || n_kept > ((size_t)1 << 36)) return fail(FMH_ERR_UNSUPPORTED, "PCA cohort too large: %zu haplotypes x %zu sites", n, n_kept);
  for (size_t i = 0; i < n_kept; ++i)
    if (h_kept_rows[i] >= m->variants) return fail(FMH_ERR_INVALID, "h_kept_rows[%zu] = %llu exceeds the matrix's %zu variants", i, (unsigned long long)h_kept_rows[i], m->variants);
  FMH_TRY(use_device(m->device));
  const bool packed = use_packed(m);
  if (!packed && !m->data) return fail(FMH_ERR_INVALID, "the matrix holds neither a packed image nor byte rows");
  Workspace* w = nullptr;
  FMH_TRY(workspace(m->device, &w));
  hipStream_t st = (hipStream_t)stream;

  const size_t n_pad = round_up(n, kPcaTile), nt = n_pad / kPcaTile, tiles = nt * (nt + 1) / 2;
  const size_t kwords = round_up((n_kept + 63) / 64, kPcaStageWords), stages = kwords / kPcaStageWords;
  // K splits: enough (tile, split) workgroups for two per CU, but a split keeps at least 8 stages (2 048 sites) so that the slab
  // traffic stays far below the multiply; FMH_PCA_SPLITS forces a count (tests: split-K on small inputs, or off)
  const long long forced = options().pca_splits.load();
  size_t splits = 1;
  if (forced > 0) splits = std::min<size_t>(std::min<size_t>((size_t)forced, stages), 65535);  // gridDim.y
  else if (tiles < 2 * (size_t)w->cus) splits = std::min<size_t>((2 * (size_t)w->cus + tiles - 1) / tiles, std::max<size_t>(stages / 8, 1));
  const size_t tile_bytes = (size_t)kPcaTile * kPcaTile * sizeof(double);
  const size_t bits_bytes = kwords * n_pad * sizeof(unsigned long long), vals_bytes = kwords * 64 * sizeof(double2);
  const size_t budget = (size_t)options().pca_budget_bytes.load();
  auto total_bytes = [&](size_t s) { return n * n * sizeof(double) + bits_bytes + vals_bytes + n_kept * 8 + (s > 1 ? s * tiles * tile_bytes : 0) + extra_bytes; };
  splits = std::min<size_t>(splits, 65535);
  // (the split count is settled against the budget here and re-derived from whole stages below, where it can only shrink)
  if (total_bytes(splits) > budget) splits = 1;
  if (total_bytes(splits) > budget)
    return fail(FMH_ERR_UNSUPPORTED, "PCA of %zu haplotypes x %zu sites needs %zu bytes of device memory, budget %zu (FMH_PCA_BUDGET_BYTES)", n, n_kept,
                total_bytes(splits), budget);
  if (check_only) return FMH_OK;
  size_t words_per_split = round_up((kwords + splits - 1) / splits, kPcaStageWords);
  splits = (kwords + words_per_split - 1) / words_per_split;

  DeviceScratch scratch(m->device, st);
  unsigned long long *d_bits = nullptr, *d_kept = nullptr;
  double2* d_vals = nullptr;
  double* d_slabs = nullptr;
  FMH_TRY(scratch.get(&d_bits, kwords * n_pad));
  FMH_TRY(scratch.get(&d_kept, n_kept));
  FMH_TRY(scratch.get(&d_vals, kwords * 64));
  if (splits > 1) FMH_TRY(scratch.get(&d_slabs, splits * tiles * (size_t)kPcaTile * kPcaTile));
  std::vector<double2> vals(kwords * 64, double2{0.0, 0.0});  // zero on the padding sites
  for (size_t i = 0; i < n_kept; ++i) vals[i] = double2{h_set_value[i], h_clear_value[i]};
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "kept rows are copied as they are");
  HIP_TRY(hipMemcpyAsync(d_kept, h_kept_rows, n_kept * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_vals, vals.data(), vals_bytes, hipMemcpyHostToDevice, st));

  // measurement: events between the three kernels (fmh_timing_enable, read back with fmh_timing_read_pca)
  KernelTimer<4> timer;
  const dim3 tgrid((unsigned)kwords, (unsigned)((n_pad / 64 + 3) / 4));
  FMH_TRY(timer.start(st));
  if (packed)
    hipLaunchKernelGGL(pca_transpose_packed_kernel, tgrid, dim3(256), 0, st, m->p0, m->plane_pitch, d_kept, n_kept, (uint32_t)n_pad, d_bits);
  else
    hipLaunchKernelGGL(pca_transpose_bytes_kernel, tgrid, dim3(256), 0, st, m->data, m->pitch, m->columns, d_kept, n_kept, (uint32_t)n_pad, d_bits);
  HIP_TRY(hipGetLastError());
  FMH_TRY(timer.mark(1, st));
  const double denom = (double)(n - 1);
  hipLaunchKernelGGL(pca_gram_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, st, d_bits, d_vals, (uint32_t)n_pad, (uint32_t)kwords,
                     (uint32_t)nt, (uint32_t)words_per_split, (uint32_t)n, denom, d_gram, d_slabs);
  HIP_TRY(hipGetLastError());
  FMH_TRY(timer.mark(2, st));
  if (splits > 1) {
    const size_t threads = tiles * (size_t)kPcaTile * kPcaTile;
    hipLaunchKernelGGL(pca_slab_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_slabs, (uint32_t)tiles, (uint32_t)splits,
                       (uint32_t)nt, (uint32_t)n, denom, d_gram);
    HIP_TRY(hipGetLastError());
  }
  FMH_TRY(timer.stop(st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  for (int i = 0; i < 3; ++i) FMH_TRY(timer.elapsed(i, &g_pca_stage_ms[i]));
  return FMH_OK;
}
}  // namespace

extern "C" int fmh_pca_gram(const fmh_matrix* m, const uint64_t* h_kept_rows, size_t n_kept, const double* h_set_value, const double* h_clear_value,
                            double* d_gram, void* stream) {
  return gram_impl(m, h_kept_rows, n_kept, h_set_value, h_clear_value, d_gram, stream, 0, false);
}

// ---- the pieces fmh_pca_gram_sharded (comm.hip) is made of ---------------------------------------------------------------------------
namespace fmhi {

int pca_gram_check(const fmh_matrix* m, const uint64_t* h_kept_rows, size_t n_kept, const double* h_set_value, const double* h_clear_value,
                   double* d_gram, size_t extra_bytes) {
  if (n_kept != 0) return gram_impl(m, h_kept_rows, n_kept, h_set_value, h_clear_value, d_gram, nullptr, extra_bytes, true);
  // a rank without kept sites contributes zeros: the matrix only says how large they are
  if (!m || !d_gram) return fail(FMH_ERR_INVALID, "NULL argument");
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "haplotype PCA needs diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  const size_t n = m->samples * 2;
  if (n < 2) return fail(FMH_ERR_INVALID, "haplotype PCA needs at least two haplotypes");
  if (n > ((size_t)1 << 24)) return fail(FMH_ERR_UNSUPPORTED, "PCA cohort too large: %zu haplotypes", n);
  const size_t need = n * n * sizeof(double) + extra_bytes, budget = (size_t)options().pca_budget_bytes.load();
  if (need > budget) return fail(FMH_ERR_UNSUPPORTED, "PCA of %zu haplotypes needs %zu bytes of device memory, budget %zu (FMH_PCA_BUDGET_BYTES)", n, need, budget);
  return FMH_OK;
}

// n x n row-major <-> its upper triangle, n (n + 1) / 2 doubles; enqueued on `st`, no synchronisation
int pca_pack_triangle(const double* d_full, size_t n, double* d_tri, hipStream_t st) {
  const size_t tiles_x = (n + kPcaTriCols - 1) / kPcaTriCols, tiles_y = (n + kPcaTriRows - 1) / kPcaTriRows;
  hipLaunchKernelGGL(pca_pack_triangle_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, st, d_full, (uint32_t)n, (uint32_t)tiles_x, d_tri);
  HIP_TRY(hipGetLastError());
  return FMH_OK;
}
int pca_unpack_triangle(const double* d_tri, size_t n, double* d_full, hipStream_t st) {
  const size_t tiles_x = (n + kPcaTriCols - 1) / kPcaTriCols, tiles_y = (n + kPcaTriRows - 1) / kPcaTriRows;
  hipLaunchKernelGGL(pca_unpack_triangle_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, st, d_tri, (uint32_t)n, (uint32_t)tiles_x, d_full);
  HIP_TRY(hipGetLastError());
  return FMH_OK;
}

}  // namespace fmhi

// The top n_components eigenpairs of the symmetric d_gram[n][n] (OVERWRITTEN) through the solver FMH_PCA_EIGEN names: lambda[k] = the k-th
// largest eigenvalue, row k of `top` its unit eigenvector.  The arguments have been checked; fmh_pca_eigen_scores and fmh_grm_eigen (grm.hip)
// share it.
int fmhi::pca_eigen_top(int device, double* d_gram, size_t n, size_t n_components, std::vector<double>& lambda, std::vector<double>& top) {
  FMH_TRY(use_device(device));
  const long long mode = options().pca_eigen.load();  // 0 = rocSOLVER, host when it cannot be loaded; 1 = host; 2 = rocSOLVER or an error
  SolverApi* api = nullptr;
  rocblas_handle handle = nullptr;
  if (mode != 1) {
    const int rc = solver_api(device, &api, &handle);
    if (rc != FMH_OK) {
      if (mode == 2) return rc;
      api = nullptr;
      static std::once_flag warned;  // the fallback is O(n^3) on one host thread: say so, once
      std::call_once(warned, [] {
        fprintf(stderr, "libferromic_hip: %s - PCA eigenproblems run on the host solver (O(n^3), one thread)\n", fmh_last_error());
      });
    }
  }
  top.assign(n_components * n, 0.0);
  lambda.assign(n_components, 0.0);
  if (api) {
    std::lock_guard<std::mutex> one_at_a_time(g_solver_device_mutex[device & 63]);
    KernelTimer<> timer;
    DeviceScratch scratch(device, nullptr);
    double *d_w = nullptr, *d_e = nullptr;
    rocblas_int* d_info = nullptr;
    FMH_TRY(scratch.get(&d_w, n));
    FMH_TRY(scratch.get(&d_e, n));
    FMH_TRY(scratch.get(&d_info, 1));
    if (api->set_stream(handle, nullptr) != 0) return fail(FMH_ERR_HIP, "rocblas_set_stream failed");
    // the matrix is symmetric, so its row-major image is its column-major image; the eigenvectors come back as COLUMNS of a
    // column-major matrix = rows of the row-major view, eigenvalues ascending
    FMH_TRY(timer.start(nullptr));
    const rocblas_status rs = api->dsyevd(handle, kEvectOriginal, kFillLower, (rocblas_int)n, d_gram, (rocblas_int)n, d_w, d_e, d_info);
    if (rs != 0) return fail(FMH_ERR_HIP, "rocsolver_dsyevd returned status %d", rs);
    FMH_TRY(timer.stop(nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    scratch.settled = true;
    FMH_TRY(timer.elapsed(0, &g_pca_stage_ms[4]));
    g_pca_stage_ms[5] = 2.0;
    rocblas_int info = 0;
    HIP_TRY(hipMemcpy(&info, d_info, sizeof info, hipMemcpyDeviceToHost));
    if (info != 0) return fail(FMH_ERR_HIP, "rocsolver_dsyevd did not converge (info %d)", (int)info);
    std::vector<double> tail(n_components * n), wv(n_components);
    HIP_TRY(hipMemcpy(tail.data(), d_gram + (n - n_components) * n, tail.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(wv.data(), d_w + (n - n_components), n_components * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n_components; ++k) {
      lambda[k] = wv[n_components - 1 - k];
      memcpy(&top[k * n], &tail[(n_components - 1 - k) * n], n * sizeof(double));
    }
  } else {
    std::vector<double> a(n * n), wv(n);
    HIP_TRY(hipMemcpy(a.data(), d_gram, a.size() * sizeof(double), hipMemcpyDeviceToHost));
    const auto t0 = std::chrono::steady_clock::now();
    eigen_symmetric_host(a.data(), n, wv.data());
    g_pca_stage_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_pca_stage_ms[5] = 1.0;
    for (size_t k = 0; k < n_components; ++k) {
      lambda[k] = wv[n - 1 - k];
      for (size_t i = 0; i < n; ++i) top[k * n + i] = a[i * n + (n - 1 - k)];
    }
  }
  return FMH_OK;
}

extern "C" int fmh_pca_eigen_scores(int device, double* d_gram, size_t n, size_t n_components, double* h_eigenvalues, double* h_scores) {
  if (!d_gram || !h_eigenvalues || !h_scores) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n < 2) return fail(FMH_ERR_INVALID, "haplotype PCA needs at least two haplotypes");
  if (n_components == 0 || n_components > n) return fail(FMH_ERR_INVALID, "n_components %zu outside 1..%zu", n_components, n);
  if (n > 46340) return fail(FMH_ERR_UNSUPPORTED, "the eigen solver takes at most 46 340 haplotypes (n * n must fit a 32-bit index), got %zu", n);
  // `top`: row k = the unit eigenvector of the k-th largest eigenvalue lambda[k]
  std::vector<double> top, lambda;
  FMH_TRY(pca_eigen_top(device, d_gram, n, n_components, lambda, top));
  // pca.rs:771-797: a column stays zero when its eigenvalue (or sigma) is not above the threshold
  for (size_t k = 0; k < n_components; ++k) {
    h_eigenvalues[k] = lambda[k];
    const double ev = std::isfinite(lambda[k]) ? std::max(lambda[k], 0.0) : 0.0;
    const double sigma = std::sqrt((double)(n - 1) * ev);
    const bool keep = ev > kNearZeroThreshold && std::isfinite(sigma) && sigma > kNearZeroThreshold;
    for (size_t i = 0; i < n; ++i) h_scores[i * n_components + k] = keep ? top[k * n + i] * sigma : 0.0;
  }
  return FMH_OK;
}
