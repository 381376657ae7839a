// pca_host.hpp — the host side of the haplotype PCA after parsing, shared by the Python module (pymodule_pca.inc) and run_vcf
// (region_driver.cpp): device scan of the sites -> the reference's f64 MAF filter and the two standardised values per kept site on the
// host (src/pca.rs:68-125, 257-290, 579-662) -> the Gram (fmh_pca_gram, or fmh_pca_gram_sharded when the sites are spread over slab
// matrices with communicators) -> fmh_pca_eigen_scores on the first slab's device; the labels and the TSV writer of pca.rs:459-463, 846-893.
// No pybind11, no run_vcf types: matrices come in as fmh_matrix handles.
#pragma once
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ferromic_hip.h"

namespace fmpca {

using std::string;
using std::vector;

// pca.rs:621: here the threshold only guards the division by a zero standard deviation, which a site that passed the MAF filter never has
constexpr double kNearZeroThreshold = FMH_PCA_NEAR_ZERO_THRESHOLD;

// a C-ABI call failed: the status and the calling thread's fmh_last_error()
struct DeviceError : std::runtime_error {
  int status;
  DeviceError(int s, const string& m) : std::runtime_error(m), status(s) {}
};
inline void check(int rc) { if (rc != FMH_OK) throw DeviceError(rc, fmh_last_error()); }

struct DeviceBlock {
  void* p = nullptr;
  int device = 0;
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
  ~DeviceBlock() { if (p) (void)fmh_device_free(device, p); }
  void alloc(int dev, size_t bytes) { device = dev; check(fmh_device_alloc(dev, bytes, &p)); }
};

// One slab of the cohort: `rows` consecutive sites starting at site `row0` of the whole, diploid, on `device`.  comm == nullptr: the
// only slab.  Otherwise every slab carries its rank's communicator of one group.
struct SlabInput {
  const fmh_matrix* m = nullptr;
  fmh_comm* comm = nullptr;
  int device = 0;
  size_t row0 = 0, rows = 0;
};

struct Output {
  size_t haplotypes = 0, components = 0;
  vector<double> coordinates;  // [haplotypes][components]
  vector<int64_t> positions;   // the kept sites
  size_t total = 0, complete = 0, kept = 0;
  double scan_seconds = 0.0, gram_seconds = 0.0, eigen_seconds = 0.0;  // wall clock, the slowest slab
};

// what the filter leaves of one slab: needs only n and the slab's own counts
struct SlabFilter {
  size_t complete = 0;
  vector<uint64_t> kept;  // rows local to the slab
  vector<double> set_value, clear_value;
};

inline SlabFilter scan_and_filter(const SlabInput& sl, size_t n, bool variant_rule) {
  SlabFilter f;
  const size_t S = sl.rows;
  if (S == 0) return f;
  DeviceBlock d_alt, d_flags;
  d_alt.alloc(sl.device, S * sizeof(uint32_t));
  d_flags.alloc(sl.device, S);
  check(fmh_pca_scan_sites(sl.m, 0, S, (uint32_t*)d_alt.p, (uint8_t*)d_flags.p, nullptr));
  vector<uint32_t> alt(S);
  vector<uint8_t> flags(S);
  check(fmh_copy_to_host(sl.device, alt.data(), d_alt.p, S * sizeof(uint32_t), nullptr));
  check(fmh_copy_to_host(sl.device, flags.data(), d_flags.p, S, nullptr));
  // the filter, pca.rs:257-290 / :68-125: the reference's f64 expression on the integer count
  for (size_t r0 = 0; r0 < S; ++r0) {
    if (flags[r0] & FMH_PCA_SITE_UNCALLED) continue;
    if (flags[r0] & FMH_PCA_SITE_HIGH_ALLELE) { if (variant_rule) ++f.complete; continue; }
    ++f.complete;
    const double freq = (double)alt[r0] / (double)n;
    const double maf = std::fmin(freq, 1.0 - freq);
    if (!(maf >= 0.05)) continue;
    f.kept.push_back(r0);
    // pca.rs:579-662: mean, variance over n - 1, scale 1 when the deviation is numerically zero
    const double mean = (double)alt[r0] / (double)n;
    const double d1 = 1.0 - mean, d0 = 0.0 - mean;
    const double var = ((double)alt[r0] * (d1 * d1) + (double)(n - alt[r0]) * (d0 * d0)) / (double)(n - 1);
    const double sd = std::sqrt(std::isfinite(var) ? std::max(var, 0.0) : 0.0);
    const double inv = 1.0 / ((!std::isfinite(sd) || sd <= kNearZeroThreshold) ? 1.0 : sd);
    f.set_value.push_back(d1 * inv);
    f.clear_value.push_back(d0 * inv);
  }
  return f;
}

// The pipeline after parsing.  `positions`: one per site of the whole cohort.  `run_on_slabs(fn)` calls fn(k) for every slab k - side
// by side when there are several (the Gram's collective needs every slab to take part at the same time) - and rethrows the first
// failure; a caller with one slab passes [](auto&& fn) { fn(0); }.  variant_rule: compute_chromosome_pca (Variant input, pca.rs:93-117)
// counts a complete site with an allele above 1 as complete; compute_chromosome_pca_from_dense (:261-268, :311-315) does not.
// false = the reference's VcfError::Parse with `*parse_error`; a failed C-ABI call throws DeviceError.
template <class RunOnSlabs>
bool compute(const vector<SlabInput>& slabs, size_t samples, const int64_t* positions, size_t n_components, bool variant_rule, RunOnSlabs&& run_on_slabs,
             Output* out, string* parse_error) {
  using clock = std::chrono::steady_clock;
  auto seconds_since = [](clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); };
  const size_t n = samples * 2;
  out->haplotypes = n;
  static const char* kNoMaf = "No variants with MAF >= 5% found for PCA";
  size_t S = 0;
  for (const SlabInput& sl : slabs) S += sl.rows;
  out->total = S;
  if (S == 0) { *parse_error = variant_rule ? "No variants provided for PCA" : kNoMaf; return false; }
  vector<SlabFilter> filters(slabs.size());
  auto t0 = clock::now();
  run_on_slabs([&](size_t k) { filters[k] = scan_and_filter(slabs[k], n, variant_rule); });
  out->scan_seconds = seconds_since(t0);
  // combined in slab order = site order
  for (size_t k = 0; k < slabs.size(); ++k) {
    out->complete += filters[k].complete;
    for (uint64_t r : filters[k].kept) out->positions.push_back(positions[slabs[k].row0 + r]);
  }
  out->kept = out->positions.size();
  if (out->kept == 0) { *parse_error = kNoMaf; return false; }
  const size_t wanted = std::min(n_components, std::min(out->complete, n));
  out->components = std::min(wanted, std::min(out->kept, n));  // pca.rs:694 / :759: min(n_components, min(m, n))
  out->coordinates.assign(n * out->components, 0.0);
  if (out->components == 0) return true;
  t0 = clock::now();
  run_on_slabs([&](size_t k) {
    const SlabInput& sl = slabs[k];
    const SlabFilter& f = filters[k];
    DeviceBlock d_gram;
    d_gram.alloc(sl.device, n * n * sizeof(double));
    if (sl.comm) check(fmh_pca_gram_sharded(sl.comm, sl.m, f.kept.data(), f.kept.size(), f.set_value.data(), f.clear_value.data(), (double*)d_gram.p, nullptr));
    else check(fmh_pca_gram(sl.m, f.kept.data(), f.kept.size(), f.set_value.data(), f.clear_value.data(), (double*)d_gram.p, nullptr));
    if (k != 0) return;  // every slab holds the sum; the first one's device solves
    out->gram_seconds = seconds_since(t0);
    const auto t1 = clock::now();
    vector<double> eigenvalues(out->components);
    check(fmh_pca_eigen_scores(sl.device, (double*)d_gram.p, n, out->components, eigenvalues.data(), out->coordinates.data()));
    out->eigen_seconds = seconds_since(t1);
  });
  return true;
}

inline vector<string> labels(const vector<string>& sample_names) {  // pca.rs:459-463
  vector<string> out;
  out.reserve(sample_names.size() * 2);
  for (const string& name : sample_names) { out.push_back(name + "_L"); out.push_back(name + "_R"); }
  return out;
}

// write_chromosome_pca_to_file, pca.rs:846-893: "Haplotype\tPC1...", one row per haplotype, "\t{:.6}" per value
inline string tsv_text(const vector<string>& labels, const double* coordinates, size_t rows, size_t components) {
  string text = "Haplotype";
  for (size_t k = 0; k < components; ++k) text += "\tPC" + std::to_string(k + 1);
  text += "\n";
  char buf[400];
  for (size_t i = 0; i < std::min(labels.size(), rows); ++i) {
    text += labels[i];
    for (size_t k = 0; k < components; ++k) {
      snprintf(buf, sizeof buf, "\t%.6f", coordinates[i * components + k]);
      text += buf;
    }
    text += "\n";
  }
  return text;
}
inline bool write_file(const std::filesystem::path& path, const string& text, string* error) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  if (f) f.write(text.data(), (std::streamsize)text.size());
  if (f) f.close();
  if (!f) { *error = string(strerror(errno)) + ": " + path.string(); return false; }
  return true;
}

}  // namespace fmpca
