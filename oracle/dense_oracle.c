/*
 * dense_oracle.c — CPU oracle, C half: literal restatement of the reference's DENSE paths
 * (src/stats.rs of SauersML/ferromic) for matrices too large for the Python restatement, plus a
 * pthread driver used as bench.py's `cpu_baseline` ("port": the reference itself is Rust and no Rust
 * toolchain exists on the build or GPU box).
 *
 * TEST INFRASTRUCTURE ONLY: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
 * may load liboracle_dense.so.  The product (libferromic_hip.so / ferromic_amd) never links,
 * imports or executes it.
 *
 * Pinning: tests/test_oracle_dense_c.py checks every function here against oracle/ferromic_ref.py,
 * which is itself pinned by the reference's own known-answer vectors (tests/golden/).
 *
 * Build: gcc -O3 -march=native -ffp-contract=off -fPIC -shared -pthread (oracle/Makefile).
 * -ffp-contract=off keeps a*b+c un-fused, as rustc does, so per-site f64 values are bit-identical
 * to the Rust expressions restated below.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define FST_EPSILON 1e-12 /* stats.rs:26 */

/* ---- counter-based synthetic cohort: identical stream to generate_kernel (sweep_kernels.hpp) ---- */
static inline uint32_t hash24(uint64_t seed, uint64_t site, uint64_t column) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (site * 0x100000001B3ull + column + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(z >> 40);
}

typedef struct {
  uint8_t* data;
  uint64_t* missing; /* may be NULL; must be zeroed by the caller */
  size_t s0, s1, variants, columns;
  uint64_t seed, first_site;
  const uint32_t* thr;
  const uint8_t* pop_of_column;
  uint32_t missing_thr;
} gen_job;

static void* gen_worker(void* p) {
  gen_job* j = (gen_job*)p;
  for (size_t s = j->s0; s < j->s1; ++s) {
    for (size_t h = 0; h < j->columns; ++h) {
      const uint32_t thr = j->thr[(size_t)j->pop_of_column[h] * j->variants + s];
      uint8_t bit = hash24(j->seed, j->first_site + s, h) < thr ? 1 : 0;
      if (j->missing && hash24(j->seed ^ 0xA5A5A5A5DEADBEEFull, j->first_site + s, h) < j->missing_thr) {
        const size_t idx = s * j->columns + h;
        __atomic_fetch_or(&j->missing[idx >> 6], 1ull << (idx & 63), __ATOMIC_RELAXED);
        bit = 0;
      }
      j->data[s * j->columns + h] = bit;
    }
  }
  return NULL;
}

/* data: [variants*columns] in the reference host layout (stats.rs:293); missing: zeroed words or NULL */
void fo_generate(uint8_t* data, uint64_t* missing, size_t variants, size_t columns, uint64_t seed,
                 uint64_t first_site, const uint32_t* thresholds24, const uint8_t* pop_of_column,
                 uint32_t missing_thr, int nthreads) {
  if (nthreads < 1) nthreads = 1;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * nthreads);
  gen_job* jobs = (gen_job*)malloc(sizeof(gen_job) * nthreads);
  for (int t = 0; t < nthreads; ++t) {
    gen_job j = {data, missing, variants * t / nthreads, variants * (t + 1) / nthreads, variants, columns,
                 seed, first_site, thresholds24, pop_of_column, missing_thr};
    jobs[t] = j;
    pthread_create(&th[t], NULL, gen_worker, &jobs[t]);
  }
  for (int t = 0; t < nthreads; ++t) pthread_join(th[t], NULL);
  free(th);
  free(jobs);
}

/* ---- stats.rs:1298-1302 ---- */
static inline int dense_missing(const uint64_t* bits, size_t idx) { return (int)((bits[idx >> 6] >> (idx & 63)) & 1); }

/* ---- stats.rs:1665-1674 ---- */
static inline size_t dense_sum_alt_no_missing(const uint8_t* data, size_t base, const size_t* offsets, size_t n_off) {
  size_t sum = 0;
  const uint8_t* ptr = data + base;
  for (size_t i = 0; i < n_off; ++i) sum += ptr[offsets[i]];
  return sum;
}

/* ---- stats.rs:1677-1697 ---- */
static inline void dense_sum_alt_with_missing(const uint8_t* data, size_t base, const size_t* offsets, size_t n_off,
                                              const uint64_t* bits, size_t* total_out, size_t* alt_out) {
  size_t alt = 0, total = 0;
  const uint8_t* ptr = data + base;
  for (size_t i = 0; i < n_off; ++i) {
    const size_t idx = base + offsets[i];
    if (dense_missing(bits, idx)) continue;
    alt += ptr[offsets[i]];
    total += 1;
  }
  *total_out = total;
  *alt_out = alt;
}

/* ---- stats.rs:1700-1709; returns 0 and leaves *out untouched for None ---- */
static inline int dense_pi_from_counts(size_t total_called, size_t alt_count, double* out) {
  if (total_called < 2) return 0;
  double n = (double)total_called;
  double alt = (double)alt_count;
  double ref_count = (double)(total_called - alt_count);
  double sum_sq = ref_count * ref_count + alt * alt;
  *out = n / (n - 1.0) * (1.0 - sum_sq / (n * n));
  return 1;
}

/* ---- stats.rs:1712-1733 ---- */
static inline int dense_dxy_from_biallelic_counts(size_t n1, size_t alt1, size_t n2, size_t alt2, double* out) {
  if (n1 == 0 || n2 == 0) return 0;
  double n1_f = (double)n1, n2_f = (double)n2;
  double alt1_f = (double)alt1 / n1_f;
  double alt2_f = (double)alt2 / n2_f;
  double ref1 = 1.0 - alt1_f;
  double ref2 = 1.0 - alt2_f;
  double dot = ref1 * ref2 + alt1_f * alt2_f;
  if (dot < 0.0) dot = 0.0;
  double dxy = 1.0 - dot;
  if (dxy < 0.0) dxy = 0.0; else if (dxy > 1.0) dxy = 1.0;
  *out = dxy;
  return 1;
}

typedef struct { /* DensePopulationSummary scalars, stats.rs:1311-1317 */
  uint64_t haplotype_capacity, segregating_sites, uncallable_sites;
  double pi_sum;
} fo_pop_totals;

typedef struct { /* HudsonSummaryTotals (1545-1552) + hudson_component_sums (1625) */
  double numerator_sum, denominator_sum, pi1_sum, pi2_sum, dxy_sum_all;
  uint64_t dxy_uncallable_sites;
  double site_num_sum, site_den_sum;
  uint64_t sites_with_components;
} fo_hudson_totals;

/*
 * build_dense_population_summary over sites [s0, s1), stats.rs:1367-1470 (one fold of the rayon arm;
 * the serial arm is the same loop over the whole range).
 */
void fo_population_summary_range(const uint8_t* data, const uint64_t* missing, size_t stride, size_t s0, size_t s1,
                                 const size_t* offsets, size_t n_off, uint32_t* alt_counts, uint32_t* called_counts,
                                 fo_pop_totals* t) {
  size_t seg = 0, unc = 0;
  double pi_total = 0.0;
  for (size_t v = s0; v < s1; ++v) {
    const size_t base = v * stride;
    size_t called, alt;
    if (missing) dense_sum_alt_with_missing(data, base, offsets, n_off, missing, &called, &alt);
    else { alt = dense_sum_alt_no_missing(data, base, offsets, n_off); called = n_off; }
    alt_counts[v] = (uint32_t)alt;
    called_counts[v] = (uint32_t)called;
    if (called >= 2 && alt > 0 && alt < called) seg += 1;
    double value;
    if (dense_pi_from_counts(called, alt, &value)) pi_total += value; else unc += 1;
  }
  t->haplotype_capacity = n_off;
  t->segregating_sites = seg;
  t->uncallable_sites = unc; /* what calculate_pi_from_summary recounts at 1512-1516 */
  t->pi_sum = pi_total;
}

/* aggregate_hudson_components_from_summaries over [s0, s1), stats.rs:1554-1623 */
void fo_hudson_from_summaries_range(const uint32_t* alt1, const uint32_t* called1, const uint32_t* alt2,
                                    const uint32_t* called2, size_t s0, size_t s1, fo_hudson_totals* t) {
  for (size_t idx = s0; idx < s1; ++idx) {
    const size_t n1 = called1[idx], n2 = called2[idx];
    if (n1 == 0 || n2 == 0) { t->dxy_uncallable_sites += 1; continue; }
    const size_t alt_count1 = alt1[idx], alt_count2 = alt2[idx];
    const size_t ref_count1 = n1 - alt_count1, ref_count2 = n2 - alt_count2;
    const double denom_pairs = (double)(n1 * n2);
    if (denom_pairs == 0.0) continue;
    double dxy = (double)(alt_count1 * ref_count2 + ref_count1 * alt_count2) / denom_pairs;
    if (dxy < 0.0) dxy = 0.0; else if (dxy > 1.0) dxy = 1.0;
    t->dxy_sum_all += dxy;
    if (n1 < 2 || n2 < 2) continue;
    const double denom1 = (double)(n1 * (n1 - 1));
    const double denom2 = (double)(n2 * (n2 - 1));
    const double pi1 = denom1 > 0.0 ? 2.0 * (double)alt_count1 * (double)ref_count1 / denom1 : 0.0;
    const double pi2 = denom2 > 0.0 ? 2.0 * (double)alt_count2 * (double)ref_count2 / denom2 : 0.0;
    t->pi1_sum += pi1;
    t->pi2_sum += pi2;
    if (dxy > FST_EPSILON) {
      t->numerator_sum += dxy - 0.5 * (pi1 + pi2);
      t->denominator_sum += dxy;
    }
  }
}

/*
 * dense_hudson_sites_biallelic over [s0, s1), stats.rs:3179-3278 (+ dense_fst_components_from_biallelic
 * 1736-1757).  Outputs are NaN for None.  Counts come from the summaries (same gather).
 */
void fo_dense_hudson_sites_biallelic_range(const uint32_t* alt1, const uint32_t* called1, const uint32_t* alt2,
                                           const uint32_t* called2, int has_missing, size_t s0, size_t s1,
                                           double* fst, double* dxy_out, double* pi1_out, double* pi2_out,
                                           double* num, double* den, fo_hudson_totals* t) {
  for (size_t v = s0; v < s1; ++v) {
    const size_t n1 = called1[v], n2 = called2[v], a1 = alt1[v], a2 = alt2[v];
    double pi1 = NAN, pi2 = NAN, dxy = NAN;
    int ok1, ok2, okd;
    if (has_missing) {
      ok1 = dense_pi_from_counts(n1, a1, &pi1);
      ok2 = dense_pi_from_counts(n2, a2, &pi2);
    } else { /* stats.rs:3219-3256 */
      ok1 = n1 >= 2;
      ok2 = n2 >= 2;
      if (ok1) {
        if (a1 == 0 || a1 == n1) pi1 = 0.0;
        else {
          double n1_f = (double)n1, scale = n1_f / (n1_f - 1.0), inv_n_sq = 1.0 / (n1_f * n1_f);
          double alt_f = (double)a1, ref_f = (double)(n1 - a1);
          pi1 = scale * (1.0 - (ref_f * ref_f + alt_f * alt_f) * inv_n_sq);
        }
      }
      if (ok2) {
        if (a2 == 0 || a2 == n2) pi2 = 0.0;
        else {
          double n2_f = (double)n2, scale = n2_f / (n2_f - 1.0), inv_n_sq = 1.0 / (n2_f * n2_f);
          double alt_f = (double)a2, ref_f = (double)(n2 - a2);
          pi2 = scale * (1.0 - (ref_f * ref_f + alt_f * alt_f) * inv_n_sq);
        }
      }
    }
    okd = dense_dxy_from_biallelic_counts(n1, a1, n2, a2, &dxy);
    double f = NAN, nc = NAN, dc = NAN;
    if (okd && ok1 && ok2) {
      if (dxy > FST_EPSILON) {
        double numv = dxy - 0.5 * (pi1 + pi2);
        f = numv / dxy; nc = numv; dc = dxy;
      } else {
        double pi_avg = 0.5 * (pi1 + pi2);
        if (fabs(pi_avg) <= FST_EPSILON) { nc = 0.0; dc = 0.0; }
      }
    }
    if (fst) fst[v] = f;
    if (dxy_out) dxy_out[v] = okd ? dxy : NAN;
    if (pi1_out) pi1_out[v] = ok1 ? pi1 : NAN;
    if (pi2_out) pi2_out[v] = ok2 ? pi2 : NAN;
    if (num) num[v] = nc;
    if (den) den[v] = dc;
    if (!isnan(nc) && !isnan(dc)) { t->site_num_sum += nc; t->site_den_sum += dc; t->sites_with_components += 1; }
  }
}

/* ---- the timed CPU baseline: "pi + Hudson FST" sweep, site ranges over pthreads ---------------- */
typedef struct {
  const uint8_t* data;
  const uint64_t* missing;
  size_t stride, s0, s1;
  const size_t *off1, *off2;
  size_t n1, n2;
  uint32_t *alt1, *called1, *alt2, *called2;
  double *fst, *dxy, *pi1, *pi2, *num, *den;
  fo_pop_totals p1, p2;
  fo_hudson_totals h;
} sweep_job;

static void* sweep_worker(void* p) {
  sweep_job* j = (sweep_job*)p;
  memset(&j->h, 0, sizeof j->h);
  /* one pass per population, as the reference does (one summary per Population object) */
  fo_population_summary_range(j->data, j->missing, j->stride, j->s0, j->s1, j->off1, j->n1, j->alt1, j->called1, &j->p1);
  fo_population_summary_range(j->data, j->missing, j->stride, j->s0, j->s1, j->off2, j->n2, j->alt2, j->called2, &j->p2);
  fo_hudson_from_summaries_range(j->alt1, j->called1, j->alt2, j->called2, j->s0, j->s1, &j->h);
  fo_dense_hudson_sites_biallelic_range(j->alt1, j->called1, j->alt2, j->called2, j->missing != NULL, j->s0, j->s1,
                                        j->fst, j->dxy, j->pi1, j->pi2, j->num, j->den, &j->h);
  return NULL;
}

/*
 * Restatement of the reference's dense Rayon algorithm for one population pair: summaries
 * (1367-1470) x2, Hudson totals from summaries (1554-1623) and the per-site records (3179-3278),
 * parallelised over site ranges like rayon's fold/reduce (partials combined in range order).
 * Per-site arrays have `variants` entries (f64 tracks may be NULL).
 */
void fo_hudson_sweep_threaded(const uint8_t* data, const uint64_t* missing, size_t variants, size_t stride,
                              const size_t* off1, size_t n1, const size_t* off2, size_t n2, uint32_t* alt1,
                              uint32_t* called1, uint32_t* alt2, uint32_t* called2, double* fst, double* dxy,
                              double* pi1, double* pi2, double* num, double* den, fo_pop_totals* pop_totals /*[2]*/,
                              fo_hudson_totals* totals, int nthreads) {
  if (nthreads < 1) nthreads = 1;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * nthreads);
  sweep_job* jobs = (sweep_job*)calloc(nthreads, sizeof(sweep_job));
  for (int t = 0; t < nthreads; ++t) {
    sweep_job* j = &jobs[t];
    j->data = data; j->missing = missing; j->stride = stride;
    j->s0 = variants * t / nthreads; j->s1 = variants * (t + 1) / nthreads;
    j->off1 = off1; j->off2 = off2; j->n1 = n1; j->n2 = n2;
    j->alt1 = alt1; j->called1 = called1; j->alt2 = alt2; j->called2 = called2;
    j->fst = fst; j->dxy = dxy; j->pi1 = pi1; j->pi2 = pi2; j->num = num; j->den = den;
    pthread_create(&th[t], NULL, sweep_worker, j);
  }
  memset(totals, 0, sizeof *totals);
  memset(pop_totals, 0, 2 * sizeof *pop_totals);
  pop_totals[0].haplotype_capacity = n1;
  pop_totals[1].haplotype_capacity = n2;
  for (int t = 0; t < nthreads; ++t) {
    pthread_join(th[t], NULL);
    sweep_job* j = &jobs[t];
    pop_totals[0].segregating_sites += j->p1.segregating_sites;
    pop_totals[0].uncallable_sites += j->p1.uncallable_sites;
    pop_totals[0].pi_sum += j->p1.pi_sum;
    pop_totals[1].segregating_sites += j->p2.segregating_sites;
    pop_totals[1].uncallable_sites += j->p2.uncallable_sites;
    pop_totals[1].pi_sum += j->p2.pi_sum;
    totals->numerator_sum += j->h.numerator_sum;
    totals->denominator_sum += j->h.denominator_sum;
    totals->pi1_sum += j->h.pi1_sum;
    totals->pi2_sum += j->h.pi2_sum;
    totals->dxy_sum_all += j->h.dxy_sum_all;
    totals->dxy_uncallable_sites += j->h.dxy_uncallable_sites;
    totals->site_num_sum += j->h.site_num_sum;
    totals->site_den_sum += j->h.site_den_sum;
    totals->sites_with_components += j->h.sites_with_components;
  }
  free(th);
  free(jobs);
}

/* ================================================================================================
 * The general twin: dense_hudson_sites_general (stats.rs:3072-3177) with dense_collect_counts (2823-2880) and the shared dot
 * product (2557-2590 / 3106-3139), the arm the reference takes for EVERY row of a matrix whose declared max_allele > 1 (3060-3070).
 * Per population: the counts of the alleles in the order they are first seen along its ascending column offsets, missing entries
 * skipped; the dot product is driven by the population with fewer distinct alleles (ties: population 1), and its terms are added in
 * that population's first-seen order.  Pinned to oracle/ferromic_ref.py bit for bit by tests/test_oracle_dense_c.py.
 * ================================================================================================ */
typedef struct {
  size_t called;
  double sum_counts_sq;
  int k;                 /* distinct alleles */
  uint8_t allele[256];   /* first-seen order */
  size_t count[256];
  int16_t slot_of[256];  /* allele -> index in allele[], -1 = not seen (reset after each row) */
} dense_counts;

static void dense_collect_counts_c(const uint8_t* data, const uint64_t* missing, size_t base, const size_t* offsets, size_t n_off, dense_counts* c) {
  c->k = 0;
  size_t called = 0;
  for (size_t i = 0; i < n_off; ++i) {
    const size_t idx = base + offsets[i];
    if (missing && dense_missing(missing, idx)) continue;
    const uint8_t a = data[idx];
    if (c->slot_of[a] < 0) { c->slot_of[a] = (int16_t)c->k; c->allele[c->k] = a; c->count[c->k] = 0; ++c->k; }
    c->count[c->slot_of[a]] += 1;
    ++called;
  }
  c->called = called; /* without missing words: every offset is called (len(offsets)) */
  double ss = 0.0;
  for (int i = 0; i < c->k; ++i) ss += (double)c->count[i] * (double)c->count[i];
  c->sum_counts_sq = ss;
}

static void dense_counts_reset(dense_counts* c) {
  for (int i = 0; i < c->k; ++i) c->slot_of[c->allele[i]] = -1;
  c->k = 0;
}

static double dense_dot_c(const dense_counts* c1, const dense_counts* c2) {
  const double inv1 = 1.0 / (double)c1->called, inv2 = 1.0 / (double)c2->called;
  double dot = 0.0;
  if (c1->k <= c2->k) {
    for (int i = 0; i < c1->k; ++i) {
      const size_t a = c1->count[i];
      if (a == 0) continue;
      const int j = c2->slot_of[c1->allele[i]];
      const size_t b = j < 0 ? 0 : c2->count[j];
      if (b != 0) dot += ((double)a * inv1) * ((double)b * inv2);
    }
  } else {
    for (int j = 0; j < c2->k; ++j) {
      const size_t b = c2->count[j];
      if (b == 0) continue;
      const int i = c1->slot_of[c2->allele[j]];
      const size_t a = i < 0 ? 0 : c1->count[i];
      if (a != 0) dot += ((double)a * inv1) * ((double)b * inv2);
    }
  }
  return dot;
}

typedef struct { /* hudson_component_sums (1625-1635) and calculate_dxy_dense's sum / skipped sites (2526-2611) */
  double site_num_sum, site_den_sum, site_dxy_sum;
  uint64_t sites_with_components, site_dxy_skipped;
} fo_hudson_general_totals;

typedef struct {
  const uint8_t* data;
  const uint64_t* missing;
  size_t stride, s0, s1;
  const size_t *off1, *off2;
  size_t n1, n2;
  uint32_t *alt1, *called1, *alt2, *called2;
  double *fst, *dxy, *pi1, *pi2, *num, *den;
  fo_pop_totals p1, p2;
  fo_hudson_general_totals h;
} general_job;

static void* general_worker(void* p) {
  general_job* j = (general_job*)p;
  dense_counts* c = (dense_counts*)malloc(2 * sizeof(dense_counts));
  if (!c) abort();
  for (int q = 0; q < 2; ++q) { memset(c[q].slot_of, 0xFF, sizeof c[q].slot_of); c[q].k = 0; }
  /* alt / called per site: build_dense_population_summary's gather (1367-1470), as the C sweep above */
  fo_pop_totals unused;
  fo_population_summary_range(j->data, j->missing, j->stride, j->s0, j->s1, j->off1, j->n1, j->alt1, j->called1, &unused);
  fo_population_summary_range(j->data, j->missing, j->stride, j->s0, j->s1, j->off2, j->n2, j->alt2, j->called2, &unused);
  memset(&j->h, 0, sizeof j->h);
  memset(&j->p1, 0, sizeof j->p1);
  memset(&j->p2, 0, sizeof j->p2);
  for (size_t v = j->s0; v < j->s1; ++v) {
    const size_t base = v * j->stride;
    dense_collect_counts_c(j->data, j->missing, base, j->off1, j->n1, &c[0]);
    dense_collect_counts_c(j->data, j->missing, base, j->off2, j->n2, &c[1]);
    const size_t n1 = c[0].called, n2 = c[1].called;
    double pi1 = NAN, pi2 = NAN, dxy = NAN;
    const int ok1 = n1 >= 2, ok2 = n2 >= 2, okd = n1 != 0 && n2 != 0;
    if (ok1) pi1 = (double)n1 / ((double)n1 - 1.0) * (1.0 - c[0].sum_counts_sq / ((double)n1 * (double)n1));
    if (ok2) pi2 = (double)n2 / ((double)n2 - 1.0) * (1.0 - c[1].sum_counts_sq / ((double)n2 * (double)n2));
    if (okd) {
      dxy = 1.0 - dense_dot_c(&c[0], &c[1]);
      if (dxy < 0.0) dxy = 0.0;
      if (dxy > 1.0) dxy = 1.0;
    }
    /* fst_components (1736-1757 == 3143-3158) */
    double f = NAN, nc = NAN, dc = NAN;
    if (okd && ok1 && ok2) {
      if (dxy > FST_EPSILON) {
        const double numv = dxy - 0.5 * (pi1 + pi2);
        f = numv / dxy; nc = numv; dc = dxy;
      } else if (fabs(0.5 * (pi1 + pi2)) <= FST_EPSILON) {
        nc = 0.0; dc = 0.0;
      }
    }
    if (j->fst) j->fst[v] = f;
    if (j->dxy) j->dxy[v] = dxy;
    if (j->pi1) j->pi1[v] = pi1;
    if (j->pi2) j->pi2[v] = pi2;
    if (j->num) j->num[v] = nc;
    if (j->den) j->den[v] = dc;
    if (!isnan(nc)) { j->h.site_num_sum += nc; j->h.site_den_sum += dc; j->h.sites_with_components += 1; }
    if (okd) j->h.site_dxy_sum += dxy; else j->h.site_dxy_skipped += 1;
    /* the general arms of count_segregating_sites_dense (3891-4084: a second allele among the called entries) and
     * calculate_pi_dense (4434-4597: pi of every site with two calls, the others skipped) */
    if (c[0].k >= 2) j->p1.segregating_sites += 1;
    if (c[1].k >= 2) j->p2.segregating_sites += 1;
    if (ok1) j->p1.pi_sum += pi1; else j->p1.uncallable_sites += 1;
    if (ok2) j->p2.pi_sum += pi2; else j->p2.uncallable_sites += 1;
    dense_counts_reset(&c[0]);
    dense_counts_reset(&c[1]);
  }
  free(c);
  return NULL;
}

/*
 * dense_hudson_sites_general over every row, site ranges over pthreads (partials combined in range order).  Per-site arrays have
 * `variants` entries (f64 tracks may be NULL; NaN = None).  alt / called: build_dense_population_summary's per-site gather (alt = the
 * SUM of the allele values; the reference builds that summary only for max_allele <= 1, so alt is the reference's only on biallelic
 * rows).  pop_totals: the general arms' segregating sites, sites with fewer than two calls, and the sum of the per-site pi.
 */
void fo_hudson_sweep_general_threaded(const uint8_t* data, const uint64_t* missing, size_t variants, size_t stride, const size_t* off1, size_t n1,
                                      const size_t* off2, size_t n2, uint32_t* alt1, uint32_t* called1, uint32_t* alt2, uint32_t* called2,
                                      double* fst, double* dxy, double* pi1, double* pi2, double* num, double* den,
                                      fo_pop_totals* pop_totals /*[2]*/, fo_hudson_general_totals* totals, int nthreads) {
  if (nthreads < 1) nthreads = 1;
  if ((size_t)nthreads > variants) nthreads = variants ? (int)variants : 1;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * nthreads);
  general_job* jobs = (general_job*)calloc(nthreads, sizeof(general_job));
  if (!th || !jobs) abort();
  for (int t = 0; t < nthreads; ++t) {
    general_job* j = &jobs[t];
    j->data = data; j->missing = missing; j->stride = stride;
    j->s0 = variants * t / nthreads; j->s1 = variants * (t + 1) / nthreads;
    j->off1 = off1; j->off2 = off2; j->n1 = n1; j->n2 = n2;
    j->alt1 = alt1; j->called1 = called1; j->alt2 = alt2; j->called2 = called2;
    j->fst = fst; j->dxy = dxy; j->pi1 = pi1; j->pi2 = pi2; j->num = num; j->den = den;
    pthread_create(&th[t], NULL, general_worker, j);
  }
  memset(totals, 0, sizeof *totals);
  memset(pop_totals, 0, 2 * sizeof *pop_totals);
  pop_totals[0].haplotype_capacity = n1;
  pop_totals[1].haplotype_capacity = n2;
  for (int t = 0; t < nthreads; ++t) {
    pthread_join(th[t], NULL);
    const general_job* j = &jobs[t];
    pop_totals[0].segregating_sites += j->p1.segregating_sites;
    pop_totals[0].uncallable_sites += j->p1.uncallable_sites;
    pop_totals[0].pi_sum += j->p1.pi_sum;
    pop_totals[1].segregating_sites += j->p2.segregating_sites;
    pop_totals[1].uncallable_sites += j->p2.uncallable_sites;
    pop_totals[1].pi_sum += j->p2.pi_sum;
    totals->site_num_sum += j->h.site_num_sum;
    totals->site_den_sum += j->h.site_den_sum;
    totals->site_dxy_sum += j->h.site_dxy_sum;
    totals->sites_with_components += j->h.sites_with_components;
    totals->site_dxy_skipped += j->h.site_dxy_skipped;
  }
  free(th);
  free(jobs);
}

/* ================================================================================================
 * Weir & Cockerham per site on a dense matrix (stats.rs:1814-2032, 2034-2127, 1781-1812) and the regional
 * sums of calculate_overall_fst_wc (2145-2374), for the full-size C3 parity gate: the Python
 * restatement (oracle/ferromic_ref.py) does ~100 sites per second, this does millions.
 * Pinned to the Python half bit for bit by tests/test_oracle_dense_c.py.
 *
 * Dense model: column h of a row is one (sample, side) entry, called unless its missing bit is set;
 * group_of_column[h] = group index or 0xFF (what SubpopulationMembership.left / right hold, 1104-1150).
 * ================================================================================================ */

/* calculate_variance_components, stats.rs:2034-2127; stats = (n_i, p_i) of the r groups with data */
static void wc_variance_components(const size_t* n, const double* p, int r_i, double global_freq, double* a_out, double* b_out) {
  const double r = (double)r_i;
  *a_out = 0.0;
  *b_out = 0.0;
  if (r < 2.0) return;
  size_t total_haplotypes = 0;
  for (int i = 0; i < r_i; ++i) total_haplotypes += n[i];
  const double n_bar = (double)total_haplotypes / r;
  if ((n_bar - 1.0) < 1e-9) return;
  const double global_p = global_freq;
  double sum_sq_diff_n = 0.0;
  for (int i = 0; i < r_i; ++i) {
    const double diff = (double)n[i] - n_bar;
    sum_sq_diff_n += diff * diff;
  }
  const double c_squared = (r > 0.0 && n_bar > 0.0) ? sum_sq_diff_n / (r * n_bar * n_bar) : 0.0;
  double numerator_s_squared = 0.0;
  for (int i = 0; i < r_i; ++i) {
    const double diff_p = p[i] - global_p;
    numerator_s_squared += (double)n[i] * diff_p * diff_p;
  }
  const double s_squared = ((r - 1.0) > 1e-9 && n_bar > 1e-9) ? numerator_s_squared / ((r - 1.0) * n_bar) : 0.0;
  const double x_wc = global_p * (1.0 - global_p) - ((r - 1.0) / r) * s_squared;
  const double a_numerator_term = s_squared - (x_wc / (n_bar - 1.0));
  const double a_denominator_factor = 1.0 - (c_squared / (r - 1.0));
  *a_out = a_numerator_term / a_denominator_factor;
  *b_out = (n_bar / (n_bar - 1.0)) * x_wc;
}

/* fst_estimate_from_components, stats.rs:1781-1812 -> 0 calculable, 1 indeterminate, 2 no variance */
static uint8_t wc_state(double a, double b) {
  const double denominator = a + b;
  if (denominator > FST_EPSILON) return 0;
  if (denominator < -FST_EPSILON) return 1;
  if (fabs(a) > FST_EPSILON) return 0;
  return 2;
}

#define FO_WC_MAX_GROUPS 32
typedef struct {
  const uint8_t* data;
  const uint64_t* missing;
  size_t stride, s0, s1, variants;
  const uint8_t* group_of_column;
  int G;
  double *a, *b; /* [slots][variants], or NULL: then only part_a / part_b / part_inf (this range's sums, site order) */
  uint8_t* state;
  double *part_a, *part_b;
  uint64_t* part_inf;
} wc_job;

static void* wc_worker(void* pv) {
  wc_job* j = (wc_job*)pv;
  const int G = j->G;
  const int slots = 1 + G * (G - 1) / 2;
  /* per-site pair slots on the heap: 32 groups make 497 slots, ~8 KB per array */
  double* pa = (double*)malloc(sizeof(double) * (size_t)slots);
  double* pb = (double*)malloc(sizeof(double) * (size_t)slots);
  uint8_t* pseen = (uint8_t*)malloc((size_t)slots);
  if (!pa || !pb || !pseen) abort();
  for (int k = 0; k < slots; ++k) { j->part_a[k] = 0.0; j->part_b[k] = 0.0; j->part_inf[k] = 0; }
  for (size_t s = j->s0; s < j->s1; ++s) {
    const size_t base = s * j->stride;
    /* alleles present among ALL called entries (1826-1837), ascending (BTreeSet) */
    uint8_t present[256];
    memset(present, 0, sizeof present);
    for (size_t h = 0; h < j->stride; ++h)
      if (!j->missing || !dense_missing(j->missing, base + h)) present[j->data[base + h]] = 1;
    double sum_a = 0.0, sum_b = 0.0;
    memset(pseen, 0, (size_t)slots);
    for (int k = 0; k < slots; ++k) { pa[k] = 0.0; pb[k] = 0.0; }
    int populated = 0;
    for (int target = 0; target < 256; ++target) {
      if (!present[target]) continue;
      size_t total_counts[FO_WC_MAX_GROUPS], alt_counts[FO_WC_MAX_GROUPS];
      for (int g = 0; g < G; ++g) { total_counts[g] = 0; alt_counts[g] = 0; }
      for (size_t h = 0; h < j->stride; ++h) {
        if (j->missing && dense_missing(j->missing, base + h)) continue;
        const uint8_t g = j->group_of_column[h];
        if (g == 0xFF) continue;
        total_counts[g] += 1;
        if (j->data[base + h] == (uint8_t)target) alt_counts[g] += 1;
      }
      size_t total_called = 0, total_target = 0, ns[FO_WC_MAX_GROUPS];
      double ps[FO_WC_MAX_GROUPS];
      int valid = 0;
      for (int g = 0; g < G; ++g) {
        if (total_counts[g] == 0) continue;
        ns[valid] = total_counts[g];
        ps[valid] = (double)alt_counts[g] / (double)total_counts[g];
        ++valid;
        total_called += total_counts[g];
        total_target += alt_counts[g];
      }
      populated = 1; /* pop_sizes_populated (1987): an allele was iterated */
      if (valid < 2) continue;
      const double global_freq = total_called > 0 ? (double)total_target / (double)total_called : 0.0;
      double ca, cb;
      wc_variance_components(ns, ps, valid, global_freq, &ca, &cb);
      sum_a += ca;
      sum_b += cb;
      int k = 1;
      for (int x = 0; x < G; ++x)
        for (int y = x + 1; y < G; ++y, ++k) {
          const size_t ta = total_counts[x], tb = total_counts[y];
          if (ta == 0 || tb == 0) continue;
          const size_t pn[2] = {ta, tb};
          const double pp[2] = {(double)alt_counts[x] / (double)ta, (double)alt_counts[y] / (double)tb};
          const size_t pair_total = ta + tb;
          const double pair_global = pair_total > 0 ? (double)(alt_counts[x] + alt_counts[y]) / (double)pair_total : 0.0;
          double qa, qb;
          wc_variance_components(pn, pp, 2, pair_global, &qa, &qb);
          pa[k] += qa;
          pb[k] += qb;
          pseen[k] = 1;
        }
    }
    for (int k = 0; k < slots; ++k) {
      /* slot 0: the overall estimate; a pair without both groups called, or a site without any allele, is insufficient (1987-2003) */
      const int has = populated && (k == 0 || pseen[k]);
      const double va = !has ? 0.0 : k == 0 ? sum_a : pa[k];
      const double vb = !has ? 0.0 : k == 0 ? sum_b : pb[k];
      const uint8_t st = has ? wc_state(va, vb) : 3;
      if (j->a) {
        const size_t o = (size_t)k * j->variants + s;
        j->a[o] = va;
        j->b[o] = vb;
        j->state[o] = st;
      } else if (st != 3) {
        j->part_a[k] += va;
        j->part_b[k] += vb;
        j->part_inf[k] += 1;
      }
    }
  }
  free(pa);
  free(pb);
  free(pseen);
  return NULL;
}

/* Per-site a, b, state for every slot (0 = overall, then pairs (0,1),(0,2),...) and the regional sums over the sites whose
 * state is not insufficient, accumulated SERIALLY in site order as the reference does (2222-2229).  a, b and state may all be
 * NULL (many groups over many sites: 26 groups make 326 slots per site): then only the sums and the informative counts, each thread's
 * site range summed in site order and the ranges added in range order (one thread: the serial sums). */
void fo_wc_sites_threaded(const uint8_t* data, const uint64_t* missing, size_t variants, size_t stride, const uint8_t* group_of_column,
                          int G, double* a, double* b, uint8_t* state, double* sum_a, double* sum_b, uint64_t* informative, int nthreads) {
  if (G < 2 || G > FO_WC_MAX_GROUPS) return;
  const int sites = a && b && state;
  if (nthreads < 1) nthreads = 1;
  if ((size_t)nthreads > variants) nthreads = variants ? (int)variants : 1;
  const int slots = 1 + G * (G - 1) / 2;
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)nthreads);
  wc_job* jobs = (wc_job*)malloc(sizeof(wc_job) * (size_t)nthreads);
  double* parts = (double*)malloc(sizeof(double) * 2 * (size_t)slots * (size_t)nthreads);
  uint64_t* parts_inf = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)slots * (size_t)nthreads);
  if (!th || !jobs || !parts || !parts_inf) abort();
  for (int t = 0; t < nthreads; ++t) {
    wc_job j = {data, missing, stride, variants * (size_t)t / (size_t)nthreads, variants * (size_t)(t + 1) / (size_t)nthreads, variants, group_of_column, G,
                sites ? a : NULL, sites ? b : NULL, sites ? state : NULL, parts + (size_t)(2 * t) * slots, parts + (size_t)(2 * t + 1) * slots,
                parts_inf + (size_t)t * slots};
    jobs[t] = j;
    pthread_create(&th[t], NULL, wc_worker, &jobs[t]);
  }
  for (int t = 0; t < nthreads; ++t) pthread_join(th[t], NULL);
  for (int k = 0; k < slots; ++k) {
    double sa = 0.0, sb = 0.0;
    uint64_t n = 0;
    if (sites) {
      for (size_t s = 0; s < variants; ++s) {
        const size_t o = (size_t)k * variants + s;
        if (state[o] != 3) { sa += a[o]; sb += b[o]; ++n; }
      }
    } else {
      for (int t = 0; t < nthreads; ++t) { sa += jobs[t].part_a[k]; sb += jobs[t].part_b[k]; n += jobs[t].part_inf[k]; }
    }
    sum_a[k] = sa;
    sum_b[k] = sb;
    informative[k] = n;
  }
  free(th);
  free(jobs);
  free(parts);
  free(parts_inf);
}

/* ================================================================================================
 * The fused region sweep (fmh_pair_region_sweep, the one call run_vcf makes per region) on a dense matrix: per site and per group the
 * called count, the distinct alleles, the alt gather (the SUM of the allele values, as fo_hudson_sweep / fo_hudson_sweep_general), the
 * per-site diversity of calculate_per_site_diversity (stats.rs:4628-4806: pi = pi_from_components 2723-2733; theta = 1 / H(n - 1) with two
 * or more distinct alleles, else 0; NaN / NaN below two calls), and - with hudson_formula = SPARSE - the six tracks of
 * hudson_site_from_variant (2969-3014: dxy_from_counts 2907-2935 adds (c1 inv1)(c2 inv2) over the shared alleles in ascending allele order,
 * then 1 - dot clamped to [0, 1]; fst_components).  hudson_formula < 0: no Hudson part.  The dense Hudson arm is fo_hudson_sweep[_general].
 *
 * Totals, in the layout of fmh_hudson_totals:
 *   pop[p]     segregating = two or more distinct alleles among the called entries, uncallable = fewer than two calls, pi_sum = the sum of
 *              the per-site pi of the sites with two calls by summary_formula: SPARSE pi_from_components; DENSE the no-missing biallelic arm
 *              (stats.rs:4485-4507) when the MATRIX has no missing words and a declared max_allele <= 1, else dense_pi_from_counts over the
 *              true sum of squared counts (1700-1709 / the general arm 4581-4584); SUMMARY dense_pi_from_counts as well (what the summary
 *              computes on a biallelic matrix).
 *   Hudson     site_num_sum / site_den_sum / sites_with_components (hudson_component_sums 1625-1635), site_dxy_sum / site_dxy_skipped
 *              (calculate_d_xy_hudson's sparse fold 2476-2496), and the fields of aggregate_hudson_components_from_summaries (1554-1623) over
 *              the alt gather (meaningful at max_allele <= 1 only).  All zero without the Hudson part.
 *
 * Model: column h of a row is one haplotype, called unless its missing bit is set, counted where it is.  A genotype whose first haplotype
 * is missing and whose second is called has no sparse form (process.rs:479-496 makes it None); it counts its called column, as the kernels
 * and the dense functions above do.  Site ranges over pthreads; each range's sums are added in range order.  Pinned to
 * oracle/ferromic_ref.py bit for bit by tests/test_oracle_dense_c.py.
 * ================================================================================================ */
#define FO_FORMULA_SPARSE 0
#define FO_FORMULA_DENSE 1
#define FO_FORMULA_SUMMARY 2

typedef struct { /* the Hudson fields of fmh_hudson_totals, in its order */
  double numerator_sum, denominator_sum, pi1_sum, pi2_sum, dxy_sum_all;
  uint64_t dxy_uncallable_sites;
  double site_num_sum, site_den_sum;
  uint64_t sites_with_components;
  double site_dxy_sum;
  uint64_t site_dxy_skipped;
} fo_region_totals;

typedef struct {
  const uint8_t* data;
  const uint64_t* missing;
  size_t stride, s0, s1, variants;
  const size_t* off[2];
  size_t n_off[2];
  const double* harmonic;
  int summary_formula, hudson_formula, nomissing_arm;
  uint32_t *alt, *called, *distinct; /* [2][variants] */
  double *site_pi, *site_theta;      /* [2][variants], may be NULL */
  double *fst, *dxy, *pi1, *pi2, *num, *den;
  fo_pop_totals p[2];
  fo_region_totals h;
} region_job;

/* pi_from_components, stats.rs:2723-2733 (n >= 2) */
static inline double fo_pi_sparse(size_t total_called, double sum_counts_sq) {
  const double n = (double)total_called;
  const double inv_n = 1.0 / n;
  const double sum_p2 = sum_counts_sq * inv_n * inv_n;
  return n / (n - 1.0) * (1.0 - sum_p2);
}

static void* region_worker(void* pv) {
  region_job* j = (region_job*)pv;
  size_t* count = (size_t*)calloc(2 * 256, sizeof(size_t));
  if (!count) abort();
  memset(&j->h, 0, sizeof j->h);
  memset(j->p, 0, sizeof j->p);
  const size_t V = j->variants;
  for (size_t v = j->s0; v < j->s1; ++v) {
    const size_t base = v * j->stride;
    size_t n[2], alt[2];
    int top = 0;
    for (int q = 0; q < 2; ++q) {
      size_t called = 0, sum = 0;
      size_t* c = count + 256 * q;
      for (size_t i = 0; i < j->n_off[q]; ++i) {
        const size_t idx = base + j->off[q][i];
        if (j->missing && dense_missing(j->missing, idx)) continue;
        const uint8_t a = j->data[idx];
        c[a] += 1;
        sum += a;
        ++called;
        if (a > top) top = a;
      }
      n[q] = called;
      alt[q] = sum;
    }
    int k[2] = {0, 0};
    double ssq[2];
    for (int q = 0; q < 2; ++q) {
      uint64_t s = 0; /* the integer sum of the squared counts: exact, so every order of the reference's additions gives these bits */
      for (int a = 0; a <= top; ++a) {
        const size_t c = count[256 * q + a];
        if (c) { ++k[q]; s += (uint64_t)c * c; }
      }
      ssq[q] = (double)s;
    }
    double pi[2];
    int ok[2];
    for (int q = 0; q < 2; ++q) {
      const size_t o = (size_t)q * V + v;
      j->alt[o] = (uint32_t)alt[q];
      j->called[o] = (uint32_t)n[q];
      j->distinct[o] = (uint32_t)k[q];
      ok[q] = n[q] >= 2;
      pi[q] = NAN;
      double tv = NAN;
      if (ok[q]) {
        pi[q] = fo_pi_sparse(n[q], ssq[q]);
        if (k[q] > 1) {
          const double denom = j->harmonic[n[q] - 1];
          tv = denom > 0.0 ? 1.0 / denom : 0.0;
        } else {
          tv = 0.0;
        }
      }
      if (j->site_pi) j->site_pi[o] = pi[q];
      if (j->site_theta) j->site_theta[o] = tv;
      /* the population summary by summary_formula */
      if (ok[q]) {
        double pv;
        if (j->summary_formula == FO_FORMULA_SPARSE) pv = pi[q];
        else if (j->summary_formula == FO_FORMULA_DENSE && j->nomissing_arm) {
          if (alt[q] == 0 || alt[q] == n[q]) pv = 0.0;
          else {
            const double nf = (double)n[q], scale = nf / (nf - 1.0), inv_n_sq = 1.0 / (nf * nf);
            const double alt_f = (double)alt[q], ref_f = (double)(n[q] - alt[q]);
            pv = scale * (1.0 - (ref_f * ref_f + alt_f * alt_f) * inv_n_sq);
          }
        } else {
          const double nf = (double)n[q];
          pv = nf / (nf - 1.0) * (1.0 - ssq[q] / (nf * nf));
        }
        j->p[q].pi_sum += pv;
      } else {
        j->p[q].uncallable_sites += 1;
      }
      if (k[q] >= 2) j->p[q].segregating_sites += 1;
    }
    if (j->hudson_formula == FO_FORMULA_SPARSE) {
      const int okd = n[0] != 0 && n[1] != 0;
      double dxy = NAN;
      if (okd) {
        const double inv1 = 1.0 / (double)n[0], inv2 = 1.0 / (double)n[1];
        double dot = 0.0;
        for (int a = 0; a <= top; ++a) {
          const size_t c1 = count[a], c2 = count[256 + a];
          if (c1 != 0 && c2 != 0) dot += ((double)c1 * inv1) * ((double)c2 * inv2);
        }
        dxy = 1.0 - dot;
        if (dxy < 0.0) dxy = 0.0;
        if (dxy > 1.0) dxy = 1.0;
      }
      double f = NAN, nc = NAN, dc = NAN; /* fst_components */
      if (okd && ok[0] && ok[1]) {
        if (dxy > FST_EPSILON) {
          const double numv = dxy - 0.5 * (pi[0] + pi[1]);
          f = numv / dxy; nc = numv; dc = dxy;
        } else if (fabs(0.5 * (pi[0] + pi[1])) <= FST_EPSILON) {
          nc = 0.0; dc = 0.0;
        }
      }
      if (j->fst) j->fst[v] = f;
      if (j->dxy) j->dxy[v] = dxy;
      if (j->pi1) j->pi1[v] = pi[0];
      if (j->pi2) j->pi2[v] = pi[1];
      if (j->num) j->num[v] = nc;
      if (j->den) j->den[v] = dc;
      if (!isnan(nc)) { j->h.site_num_sum += nc; j->h.site_den_sum += dc; j->h.sites_with_components += 1; }
      if (okd) j->h.site_dxy_sum += dxy; else j->h.site_dxy_skipped += 1;
    }
    for (int q = 0; q < 2; ++q)
      for (int a = 0; a <= top; ++a) count[256 * q + a] = 0;
  }
  if (j->hudson_formula == FO_FORMULA_SPARSE) {
    fo_hudson_totals s;
    memset(&s, 0, sizeof s);
    fo_hudson_from_summaries_range(j->alt, j->called, j->alt + V, j->called + V, j->s0, j->s1, &s);
    j->h.numerator_sum = s.numerator_sum;
    j->h.denominator_sum = s.denominator_sum;
    j->h.pi1_sum = s.pi1_sum;
    j->h.pi2_sum = s.pi2_sum;
    j->h.dxy_sum_all = s.dxy_sum_all;
    j->h.dxy_uncallable_sites = s.dxy_uncallable_sites;
  }
  free(count);
  return NULL;
}

/* Returns 0, or -1 for a formula outside the model (summary_formula not SPARSE / DENSE / SUMMARY, hudson_formula not SPARSE or < 0).
 * alt, called, distinct: [2][variants] (required); site_pi, site_theta: [2][variants]; the six Hudson tracks: [variants] (all nullable). */
int fo_region_sweep_threaded(const uint8_t* data, const uint64_t* missing, size_t variants, size_t stride, int max_allele, const size_t* off1,
                             size_t n1, const size_t* off2, size_t n2, int summary_formula, int hudson_formula, uint32_t* alt, uint32_t* called,
                             uint32_t* distinct, double* site_pi, double* site_theta, double* fst, double* dxy, double* pi1, double* pi2,
                             double* num, double* den, fo_pop_totals* pop_totals /*[2]*/, fo_region_totals* totals, int nthreads) {
  if (summary_formula < FO_FORMULA_SPARSE || summary_formula > FO_FORMULA_SUMMARY) return -1;
  if (hudson_formula >= 0 && hudson_formula != FO_FORMULA_SPARSE) return -1;
  if (nthreads < 1) nthreads = 1;
  if ((size_t)nthreads > variants) nthreads = variants ? (int)variants : 1;
  /* H_k = sum_{i=1..k} 1/i added in ascending order, harmonic() (stats.rs:4234-4240) */
  const size_t max_n = n1 > n2 ? n1 : n2;
  double* harmonic = (double*)malloc(sizeof(double) * (max_n + 1));
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)nthreads);
  region_job* jobs = (region_job*)calloc((size_t)nthreads, sizeof(region_job));
  if (!harmonic || !th || !jobs) abort();
  double hs = 0.0;
  harmonic[0] = 0.0;
  for (size_t k = 1; k <= max_n; ++k) {
    hs += 1.0 / (double)k;
    harmonic[k] = hs;
  }
  for (int t = 0; t < nthreads; ++t) {
    region_job* j = &jobs[t];
    j->data = data; j->missing = missing; j->stride = stride; j->variants = variants;
    j->s0 = variants * (size_t)t / (size_t)nthreads; j->s1 = variants * (size_t)(t + 1) / (size_t)nthreads;
    j->off[0] = off1; j->off[1] = off2; j->n_off[0] = n1; j->n_off[1] = n2;
    j->harmonic = harmonic;
    j->summary_formula = summary_formula; j->hudson_formula = hudson_formula;
    j->nomissing_arm = missing == NULL && max_allele <= 1;
    j->alt = alt; j->called = called; j->distinct = distinct; j->site_pi = site_pi; j->site_theta = site_theta;
    j->fst = fst; j->dxy = dxy; j->pi1 = pi1; j->pi2 = pi2; j->num = num; j->den = den;
    pthread_create(&th[t], NULL, region_worker, j);
  }
  memset(totals, 0, sizeof *totals);
  memset(pop_totals, 0, 2 * sizeof *pop_totals);
  pop_totals[0].haplotype_capacity = n1;
  pop_totals[1].haplotype_capacity = n2;
  for (int t = 0; t < nthreads; ++t) {
    pthread_join(th[t], NULL);
    const region_job* j = &jobs[t];
    for (int q = 0; q < 2; ++q) {
      pop_totals[q].segregating_sites += j->p[q].segregating_sites;
      pop_totals[q].uncallable_sites += j->p[q].uncallable_sites;
      pop_totals[q].pi_sum += j->p[q].pi_sum;
    }
    totals->numerator_sum += j->h.numerator_sum;
    totals->denominator_sum += j->h.denominator_sum;
    totals->pi1_sum += j->h.pi1_sum;
    totals->pi2_sum += j->h.pi2_sum;
    totals->dxy_sum_all += j->h.dxy_sum_all;
    totals->dxy_uncallable_sites += j->h.dxy_uncallable_sites;
    totals->site_num_sum += j->h.site_num_sum;
    totals->site_den_sum += j->h.site_den_sum;
    totals->sites_with_components += j->h.sites_with_components;
    totals->site_dxy_sum += j->h.site_dxy_sum;
    totals->site_dxy_skipped += j->h.site_dxy_skipped;
  }
  free(harmonic);
  free(th);
  free(jobs);
  return 0;
}

/* ---- all-pairs differences (calculate_pairwise_differences, stats.rs:4106-4231) on a dense matrix, bit-parallel on haplotypes ------
 * For samples i < j < n_samples over every site:
 *   diff(i, j) = number of (a, b), a an allele of genotype i and b one of genotype j, with a != b, at sites where both are Some
 *   both(i, j) = number of sites where both genotypes are Some
 * where a sample's genotype at a site is the prefix of its called alleles (CompressedGenotypes::get, process.rs:479-496): slot k is
 * EFFECTIVE iff slots 0..k are all called, and the genotype is Some iff slot 0 is effective.
 * The matrix is transposed once to haplotype-major words of 64 sites - one word row per bit of the allele value and one for the
 * effective bit e - and then
 *   diff(i, j) = sum_{a, b < ploidy} popcount( OR_bits(h_ia ^ h_jb) & e_ia & e_jb ),   both(i, j) = popcount(e_i0 & e_j0).
 * No allele counts, no products: deliberately not the algebra of the device kernels it checks.
 * Layout: T[block][haplotype][plane][PD_BW words], planes = allele bits then e; a block (PD_BW * 64 sites of every haplotype) is what the
 * pair loop keeps in cache.  Threads own disjoint sets of (sample tile, sample tile) pairs and walk the blocks in the same order. */
#define PD_BW 64
#define PD_TILE 32

typedef struct {
  const uint8_t* data;
  const uint64_t* missing;
  size_t variants, stride, ploidy, n_samples, blocks;
  int planes; /* allele bits + 1 */
  uint64_t* T;
  uint64_t* tmp; /* this thread's P * H words of the transpose */
  uint64_t *diff, *both;
  int t, nthreads;
} pd_job;

static void* pd_transpose_worker(void* pv) {
  pd_job* j = (pd_job*)pv;
  const size_t H = j->n_samples * j->ploidy, P = (size_t)j->planes, nbits = P - 1;
  const size_t words = (j->variants + 63) / 64;
  const size_t w0 = words * (size_t)j->t / (size_t)j->nthreads, w1 = words * ((size_t)j->t + 1) / (size_t)j->nthreads;
  uint64_t* tmp = j->tmp;
  for (size_t w = w0; w < w1; ++w) {
    memset(tmp, 0, sizeof(uint64_t) * P * H);
    for (size_t s = 0; s < 64 && w * 64 + s < j->variants; ++s) {
      const size_t base = (w * 64 + s) * j->stride;
      for (size_t smp = 0; smp < j->n_samples; ++smp) {
        uint64_t eff = 1;
        for (size_t k = 0; k < j->ploidy; ++k) {
          const size_t h = smp * j->ploidy + k;
          if (j->missing) eff &= (uint64_t)!dense_missing(j->missing, base + h);
          const uint64_t v = j->data[base + h] & (0 - eff);
          for (size_t b = 0; b < nbits; ++b) tmp[h * P + b] |= ((v >> b) & 1u) << s;
          tmp[h * P + nbits] |= eff << s;
        }
      }
    }
    uint64_t* blk = j->T + (w / PD_BW) * H * P * PD_BW + (w % PD_BW);
    for (size_t hp = 0; hp < H * P; ++hp) blk[hp * PD_BW] = tmp[hp];
  }
  return NULL;
}

static void* pd_pairs_worker(void* pv) {
  pd_job* j = (pd_job*)pv;
  const size_t n = j->n_samples, pl = j->ploidy, P = (size_t)j->planes, nbits = P - 1, H = n * pl;
  const size_t tiles = (n + PD_TILE - 1) / PD_TILE;
  for (size_t blk = 0; blk < j->blocks; ++blk) {
    const uint64_t* B = j->T + blk * H * P * PD_BW;
    size_t tp = 0;
    for (size_t ti = 0; ti < tiles; ++ti)
      for (size_t tj = ti; tj < tiles; ++tj, ++tp) {
        if (tp % (size_t)j->nthreads != (size_t)j->t) continue;
        const size_t i1 = (ti + 1) * PD_TILE < n ? (ti + 1) * PD_TILE : n, j1 = (tj + 1) * PD_TILE < n ? (tj + 1) * PD_TILE : n;
        for (size_t i = ti * PD_TILE; i < i1; ++i)
          for (size_t jj = (tj == ti ? i + 1 : tj * PD_TILE); jj < j1; ++jj) {
            uint64_t d = 0, bo = 0;
            const uint64_t *ei0 = B + ((i * pl) * P + nbits) * PD_BW, *ej0 = B + ((jj * pl) * P + nbits) * PD_BW;
            for (size_t w = 0; w < PD_BW; ++w) bo += (uint64_t)__builtin_popcountll(ei0[w] & ej0[w]);
            for (size_t a = 0; a < pl; ++a) {
              const uint64_t* x = B + ((i * pl + a) * P) * PD_BW;
              for (size_t b = 0; b < pl; ++b) {
                const uint64_t* y = B + ((jj * pl + b) * P) * PD_BW;
                if (nbits == 1) {
                  for (size_t w = 0; w < PD_BW; ++w)
                    d += (uint64_t)__builtin_popcountll((x[w] ^ y[w]) & x[PD_BW + w] & y[PD_BW + w]);
                } else {
                  for (size_t w = 0; w < PD_BW; ++w) {
                    uint64_t ne = 0;
                    for (size_t q = 0; q < nbits; ++q) ne |= x[q * PD_BW + w] ^ y[q * PD_BW + w];
                    d += (uint64_t)__builtin_popcountll(ne & x[nbits * PD_BW + w] & y[nbits * PD_BW + w]);
                  }
                }
              }
            }
            j->diff[i * n + jj] += d;
            j->both[i * n + jj] += bo;
          }
      }
  }
  return NULL;
}

/* data: [variants][stride] u8 (site-major, sample s = columns s * ploidy .. + ploidy - 1), missing: bit (site * stride + column) or NULL.
 * diff, both: [n_samples][n_samples] u64, zeroed here, upper triangle filled.  Returns 0, or -1 when out of memory. */
int fo_pairwise_differences_threaded(const uint8_t* data, const uint64_t* missing, size_t variants, size_t stride, size_t ploidy,
                                     size_t n_samples, int max_allele, uint64_t* diff, uint64_t* both, int nthreads) {
  memset(diff, 0, sizeof(uint64_t) * n_samples * n_samples);
  memset(both, 0, sizeof(uint64_t) * n_samples * n_samples);
  if (n_samples < 2 || variants == 0 || ploidy == 0) return 0;
  if (nthreads < 1) nthreads = 1;
  int nbits = 1;
  while (nbits < 8 && (max_allele >> nbits) != 0) ++nbits;
  const size_t words = (variants + 63) / 64, blocks = (words + PD_BW - 1) / PD_BW;
  const size_t H = n_samples * ploidy, P = (size_t)nbits + 1;
  uint64_t* T = (uint64_t*)calloc(blocks * H * P * PD_BW, sizeof(uint64_t)); /* words past the last site stay 0: e = 0 there */
  uint64_t* tmp = (uint64_t*)malloc(sizeof(uint64_t) * P * H * (size_t)nthreads);
  pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)nthreads);
  pd_job* jobs = (pd_job*)malloc(sizeof(pd_job) * (size_t)nthreads);
  int* started = (int*)malloc(sizeof(int) * (size_t)nthreads);
  if (!T || !tmp || !th || !jobs || !started) {
    free(T); free(tmp); free(th); free(jobs); free(started);
    return -1;
  }
  for (int t = 0; t < nthreads; ++t) {
    pd_job j = {data, missing, variants, stride, ploidy, n_samples, blocks, (int)P, T, tmp + (size_t)t * P * H, diff, both, t, nthreads};
    jobs[t] = j;
  }
  void* (*phases[2])(void*) = {pd_transpose_worker, pd_pairs_worker};
  for (int ph = 0; ph < 2; ++ph) { /* a thread that cannot be started: its share runs here, the result is the same */
    for (int t = 0; t < nthreads; ++t) started[t] = pthread_create(&th[t], NULL, phases[ph], &jobs[t]) == 0;
    for (int t = 0; t < nthreads; ++t) {
      if (started[t]) pthread_join(th[t], NULL);
      else phases[ph](&jobs[t]);
    }
  }
  free(started);
  free(th);
  free(jobs);
  free(tmp);
  free(T);
  return 0;
}
