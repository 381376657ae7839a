// Part of pymodule.cpp: result classes, Population, path selection (src/stats.rs) and the module definition.
namespace {

// ---------------------------------------------------------------------------------------------------------------
// sweeps (thin typed wrappers over the C-ABI; the GIL is released while the GPU works)
// ---------------------------------------------------------------------------------------------------------------
vector<fmh_pop_totals> sweep_summaries(const DevMatrix& m, const vector<vector<uint8_t>>& masks, int formula, size_t r0, size_t rc,
                                       vector<uint32_t>* alt = nullptr, vector<uint32_t>* called = nullptr) {
  const shared_ptr<Groups> gp = groups_for(m, masks);
  Groups& g = *gp;
  const size_t P = masks.size();
  std::unique_ptr<DevBuf> d_alt, d_called;
  if (alt) d_alt.reset(new DevBuf(m.device, 4 * P * rc));
  if (called) d_called.reset(new DevBuf(m.device, 4 * P * rc));
  vector<fmh_pop_totals> totals(P);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_population_summaries(m.h, g.h, r0, rc, formula, d_alt ? (uint32_t*)d_alt->p : nullptr, d_called ? (uint32_t*)d_called->p : nullptr,
                                      totals.data(), nullptr);
  }
  fmh_check(status);
  if (alt) *alt = d_alt->fetch<uint32_t>(P * rc);
  if (called) *called = d_called->fetch<uint32_t>(P * rc);
  return totals;
}

struct HudsonOut {
  fmh_hudson_totals t;
  bool have_sites = false;
  vector<double> fst, dxy, pi1, pi2, num, den;
  vector<uint32_t> called;  // [2][rows]
};

HudsonOut sweep_hudson(const DevMatrix& m, const vector<uint8_t>& mask1, const vector<uint8_t>& mask2, int formula, size_t r0, size_t rc,
                       bool want_sites) {
  const shared_ptr<Groups> gp = groups_for(m, {mask1, mask2});
  Groups& g = *gp;
  HudsonOut out;
  memset(&out.t, 0, sizeof out.t);
  std::unique_ptr<DevBuf> b[6], b_called;
  fmh_hudson_sites sites;
  memset(&sites, 0, sizeof sites);
  if (want_sites) {
    for (auto& x : b) x.reset(new DevBuf(m.device, 8 * rc));
    b_called.reset(new DevBuf(m.device, 4 * 2 * rc));
    sites.d_fst = (double*)b[0]->p; sites.d_dxy = (double*)b[1]->p; sites.d_pi1 = (double*)b[2]->p; sites.d_pi2 = (double*)b[3]->p;
    sites.d_num = (double*)b[4]->p; sites.d_den = (double*)b[5]->p; sites.d_called = (uint32_t*)b_called->p;
  }
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_hudson_sweep(m.h, g.h, r0, rc, formula, want_sites ? &sites : nullptr, &out.t, nullptr);
  }
  fmh_check(status);
  if (want_sites) {
    out.have_sites = true;
    out.fst = b[0]->fetch<double>(rc); out.dxy = b[1]->fetch<double>(rc); out.pi1 = b[2]->fetch<double>(rc);
    out.pi2 = b[3]->fetch<double>(rc); out.num = b[4]->fetch<double>(rc); out.den = b[5]->fetch<double>(rc);
    out.called = b_called->fetch<uint32_t>(2 * rc);
  }
  return out;
}

struct WcOut {
  size_t G = 0, nw = 0, rows = 0;
  vector<double> sum_a, sum_b;
  vector<uint64_t> informative;
  vector<double> a, b;          // [nw][rows]
  vector<uint8_t> state;        // [nw][rows]
  vector<uint32_t> group_called;  // [G][rows]
};

WcOut sweep_wc(const DevMatrix& m, const vector<vector<uint8_t>>& masks, size_t r0, size_t rc) {
  WcOut o;
  o.G = masks.size();
  o.nw = 1 + o.G * (o.G - 1) / 2;
  o.rows = rc;
  DevBuf d_a(m.device, 8 * o.nw * rc), d_b(m.device, 8 * o.nw * rc), d_s(m.device, o.nw * rc), d_n(m.device, 4 * o.G * rc);
  o.sum_a.assign(o.nw, 0.0); o.sum_b.assign(o.nw, 0.0); o.informative.assign(o.nw, 0);
  int status;
  if (o.G <= FMH_MAX_GROUPS) {  // the fused sweep; beyond 8 groups: counting sweeps in batches + the counts kernel (same per-site bits)
    const shared_ptr<Groups> gp = groups_for(m, masks);
    Groups& g = *gp;
    fmh_wc_totals t;
    {
      py::gil_scoped_release nogil;
      status = fmh_wc_sweep(m.h, g.h, r0, rc, (double*)d_a.p, (double*)d_b.p, (uint8_t*)d_s.p, (uint32_t*)d_n.p, &t, nullptr);
    }
    fmh_check(status);
    for (size_t k = 0; k < o.nw; ++k) { o.sum_a[k] = t.sum_a[k]; o.sum_b[k] = t.sum_b[k]; o.informative[k] = t.informative_sites[k]; }
  } else {
    vector<uint8_t> flat;
    for (auto& k : masks) flat.insert(flat.end(), k.begin(), k.end());
    {
      py::gil_scoped_release nogil;
      status = fmh_wc_sweep_many(m.h, flat.data(), (int)o.G, r0, rc, (double*)d_a.p, (double*)d_b.p, (uint8_t*)d_s.p, (uint32_t*)d_n.p,
                                 o.sum_a.data(), o.sum_b.data(), o.informative.data(), nullptr);
    }
    fmh_check(status);
  }
  o.a = d_a.fetch<double>(o.nw * rc);
  o.b = d_b.fetch<double>(o.nw * rc);
  o.state = d_s.fetch<uint8_t>(o.nw * rc);
  o.group_called = d_n.fetch<uint32_t>(o.G * rc);
  return o;
}

// ---------------------------------------------------------------------------------------------------------------
// result classes (lib.rs:75-545): read-only attributes, the reference's reprs
// ---------------------------------------------------------------------------------------------------------------
string fmt6(double v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%.6f", v);
  return buf;
}
string optional_float_display(const optional<double>& v) {  // lib.rs:817-823
  if (!v) return "None";
  if (std::isfinite(*v)) return fmt6(*v);
  return std::isnan(*v) ? "NaN" : (*v > 0 ? "inf" : "-inf");
}
string rust_debug_opt(const py::object& v) {  // Option<T> Debug
  if (v.is_none()) return "None";
  return "Some(" + py::cast<string>(py::repr(v)) + ")";
}
py::object opt_to_py(const optional<double>& v) { return v ? py::object(py::float_(*v)) : py::object(py::none()); }

static const char* kWcStates[4] = {"calculable", "components_yield_indeterminate_ratio", "no_inter_population_variance",
                                   "insufficient_data_for_estimation"};

struct FstEstimate {  // lib.rs:76-165
  string state;
  py::object value, sum_a, sum_b, sites;
  py::tuple components() const { return py::make_tuple(value, sum_a, sum_b, sites); }
  string repr() const {
    string v = value.is_none() ? "None" : fmt6(py::cast<double>(value));
    return "FstEstimate(state='" + state + "', value=" + v + ", sum_a=" + rust_debug_opt(sum_a) + ", sum_b=" + rust_debug_opt(sum_b) +
           ", sites=" + rust_debug_opt(sites) + ")";
  }
};

double ieee_div(double x, double y) { return x / y; }  // IEEE semantics incl. division by zero (Rust f64 `/`)

// fst_estimate_from_components (stats.rs:1781-1812) / regional ladder (2234-2270)
FstEstimate classify(double a, double b, size_t sites) {
  const double denominator = a + b;
  FstEstimate e;
  e.sum_a = py::float_(a); e.sum_b = py::float_(b); e.sites = py::int_(sites);
  if (denominator > kFstEpsilon) { e.state = kWcStates[0]; e.value = py::float_(ieee_div(a, denominator)); return e; }
  if (denominator < -kFstEpsilon) { e.state = kWcStates[1]; e.value = py::none(); return e; }
  if (std::fabs(a) > kFstEpsilon) { e.state = kWcStates[0]; e.value = py::float_(ieee_div(a, denominator)); return e; }
  e.state = kWcStates[2]; e.value = py::none();
  return e;
}
FstEstimate insufficient(size_t sites) {
  FstEstimate e;
  e.state = kWcStates[3]; e.value = py::none(); e.sum_a = py::float_(0.0); e.sum_b = py::float_(0.0); e.sites = py::int_(sites);
  return e;
}

struct PairwiseDifference {
  int64_t sample_i, sample_j;
  py::object differences, comparable_sites;  // arbitrary-size ints (L * h_i * h_j can exceed 64 bits in principle)
  string repr() const {
    return "PairwiseDifference(sample_i=" + std::to_string(sample_i) + ", sample_j=" + std::to_string(sample_j) + ", differences=" +
           py::cast<string>(py::str(differences)) + ", comparable_sites=" + py::cast<string>(py::str(comparable_sites)) + " [genomic bases])";
  }
};

#include "pymodule_pca.inc"

struct DiversitySite {
  int64_t position;
  double pi, watterson_theta;
  string repr() const {
    return "DiversitySite(position=" + std::to_string(position) + ", pi=" + fmt6(pi) + ", watterson_theta=" + fmt6(watterson_theta) + ")";
  }
};

struct HudsonDxyResult {
  optional<double> d_xy;
  string repr() const { return d_xy ? "HudsonDxyResult(d_xy=" + fmt6(*d_xy) + ")" : "HudsonDxyResult(d_xy=None)"; }
};

struct HudsonFstSite {
  int64_t position;
  optional<double> fst, d_xy, pi_pop1, pi_pop2;
  int64_t n1_called, n2_called;
  optional<double> numerator_component, denominator_component;
  string repr() const {
    return "HudsonFstSite(position=" + std::to_string(position) + ", fst=" + optional_float_display(fst) + ", d_xy=" + optional_float_display(d_xy) +
           ", pi_pop1=" + optional_float_display(pi_pop1) + ", pi_pop2=" + optional_float_display(pi_pop2) + ", n1_called=" +
           std::to_string(n1_called) + ", n2_called=" + std::to_string(n2_called) + ")";
  }
};

struct HudsonFstResult {
  optional<double> fst, d_xy, pi_pop1, pi_pop2, pi_xy_avg;
  py::object population1_label, population1_haplotype_group, population2_label, population2_haplotype_group;
  string repr() const {
    auto lab = [](const py::object& l) { return l.is_none() || py::len(l) == 0 ? string("<unknown>") : py::cast<string>(l); };
    return "HudsonFstResult(fst=" + optional_float_display(fst) + ", d_xy=" + optional_float_display(d_xy) + ", pi_pop1=" +
           optional_float_display(pi_pop1) + ", pi_pop2=" + optional_float_display(pi_pop2) + ", pi_xy_avg=" + optional_float_display(pi_xy_avg) +
           ", pop1=" + lab(population1_label) + ", pop2=" + lab(population2_label) + ")";
  }
};

struct WcFstSite {
  int64_t position;
  FstEstimate overall_fst;
  py::dict pairwise_fst;
  double variance_components_a, variance_components_b;
  py::dict population_sizes, pairwise_variance_components;
  string repr() const { return "WcFstSite(position=" + std::to_string(position) + ", overall_fst=" + overall_fst.repr() + ")"; }
};

struct WcFstResult {
  FstEstimate overall_fst;
  py::dict pairwise_fst, pairwise_variance_components;
  py::list site_fst;
  string fst_type;
  string repr() const { return "WcFstResult(overall_fst=" + overall_fst.repr() + ")"; }
};

void population_label(const PopId& id, py::object* label, py::object* group) {  // lib.rs:1393-1400
  if (id.is_group) { *label = py::str("haplotype_group_" + std::to_string(id.group)); *group = py::int_(id.group); }
  else { *label = py::str(id.name); *group = py::none(); }
}

// ---------------------------------------------------------------------------------------------------------------
// Population (lib.rs:547-814)
// ---------------------------------------------------------------------------------------------------------------
struct Population {
  PopId id;
  shared_ptr<const Store> store;
  vector<Hap> haplotypes;
  vector<string> sample_names;
  int64_t sequence_length = 0;
  shared_ptr<Dense> dense;
  mutable optional<fmh_pop_totals> summary;  // OnceLock, lib.rs:738
  // the per-site half of the reference's DensePopulationSummary (alt_counts / called_counts, stats.rs:1367-1470), kept on the device: what
  // a Hudson pair with a population of ANOTHER matrix is computed from (fmh_hudson_from_counts); built on first use
  struct SiteCounts { std::unique_ptr<DevBuf> alt, called; size_t rows = 0; int device = 0; };
  mutable shared_ptr<SiteCounts> site_counts;
  const SiteCounts& dense_site_counts() const {
    if (!site_counts) {
      auto dm = dense->device_matrix();
      auto sc = std::make_shared<SiteCounts>();
      sc->rows = dm->variants; sc->device = dm->device;
      sc->alt.reset(new DevBuf(dm->device, 4 * sc->rows));
      sc->called.reset(new DevBuf(dm->device, 4 * sc->rows));
      fmh_pop_totals tot;
      memset(&tot, 0, sizeof tot);
      if (sc->rows) {
        const shared_ptr<Groups> gp = groups_for(*dm, {dense->mask_for(haplotypes)});
        Groups& g = *gp;
        int status;
        {
          py::gil_scoped_release nogil;
          status = fmh_population_summaries(dm->h, g.h, 0, sc->rows, FMH_FORMULA_SUMMARY, (uint32_t*)sc->alt->p, (uint32_t*)sc->called->p, &tot, nullptr);
        }
        fmh_check(status);
        if (!summary) summary = tot;
      }
      site_counts = sc;
    }
    return *site_counts;
  }

  // as_population_context, lib.rs:777-799: the summary exists only for a diploid biallelic dense matrix
  const fmh_pop_totals* dense_summary() const {
    if (!dense || dense->max_allele > 1) return nullptr;
    if (!summary) {
      auto dm = dense->device_matrix();
      summary = sweep_summaries(*dm, {dense->mask_for(haplotypes)}, FMH_FORMULA_SUMMARY, 0, dm->variants)[0];
    }
    return &*summary;
  }
  string repr() const {
    const string label = id.is_group ? "haplotype_group " + std::to_string(id.group) : "named '" + id.name + "'";
    return "Population(" + label + ", haplotypes=" + std::to_string(haplotypes.size()) + ", variants=" + std::to_string(store->S) +
           ", sequence_length=" + std::to_string(sequence_length) + ")";
  }
};

vector<string> to_string_list(const py::handle& obj) {
  vector<string> out;
  if (obj.is_none()) return out;
  for (py::handle x : py::reinterpret_borrow<py::object>(obj)) out.push_back(py::cast<string>(py::str(x)));
  return out;
}

shared_ptr<Population> make_population(const PopId& id, shared_ptr<const Store> store, vector<Hap> haps, vector<string> names, int64_t L,
                                       shared_ptr<Dense> dense) {
  auto p = std::make_shared<Population>();
  p->id = id; p->store = std::move(store); p->haplotypes = std::move(haps); p->sample_names = std::move(names);
  p->sequence_length = L; p->dense = std::move(dense);
  return p;
}

int64_t positive_length(const py::handle& obj) {
  const int64_t L = to_i64(obj);
  if (L <= 0) value_error("sequence_length must be a positive integer");
  return L;
}

// PopulationInput::extract, lib.rs:978-1080
shared_ptr<Population> coerce_population(const py::handle& obj) {
  if (py::isinstance<Population>(obj)) return py::cast<shared_ptr<Population>>(obj);
  if (py::isinstance<py::dict>(obj)) {
    py::dict d = py::reinterpret_borrow<py::dict>(obj);
    const PopId id = parse_population_id(mapping_field(d, {"id", "population_id", "name"}));
    if (!d.contains("variants")) value_error("population requires 'variants'");
    if (!d.contains("haplotypes")) value_error("population requires 'haplotypes'");
    const int64_t L = positive_length(mapping_field(d, {"sequence_length", "length", "L"}));
    vector<string> names = d.contains("sample_names") ? to_string_list(d["sample_names"]) : vector<string>();
    return make_population(id, store_from_python(d["variants"]), parse_haplotypes(d["haplotypes"]), names, L, nullptr);
  }
  py::object pid = field(obj, {"id", "population_id", "name"});
  if (pid.is_none()) value_error("population-like object missing 'id'");
  py::object variants = field(obj, {"variants"});
  if (variants.is_none()) value_error("population-like object missing 'variants'");
  py::object haplotypes = field(obj, {"haplotypes"});
  if (haplotypes.is_none()) value_error("population-like object missing 'haplotypes'");
  py::object L = field(obj, {"sequence_length", "length", "L"});
  if (L.is_none()) value_error("population-like object missing 'sequence_length'");
  const int64_t len = positive_length(L);
  py::object names = field(obj, {"sample_names", "samples"});
  return make_population(parse_population_id(pid), store_from_python(variants), parse_haplotypes(haplotypes), to_string_list(names), len, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------
// statistics: path selection mirrors src/stats.rs, arithmetic runs on the GPU
// ---------------------------------------------------------------------------------------------------------------
fmh_pop_totals empty_totals(const vector<uint8_t>& mask) {
  fmh_pop_totals t;
  memset(&t, 0, sizeof t);
  t.haplotype_capacity = mask_count(mask);
  return t;
}

// population-summary sweep over the sparse model (FORMULA_SPARSE)
fmh_pop_totals sparse_pop_sweep(const Store& store, const vector<uint8_t>& mask) {
  if (store.S == 0) return empty_totals(mask);
  auto [dm, r0, rc] = store.device_rows();
  return sweep_summaries(*dm, {mask}, FMH_FORMULA_SPARSE, r0, rc)[0];
}

// count_segregating_sites_for_population, stats.rs:3831-3851
uint64_t count_segregating_sites_for_population(const Population& pop) {
  if (const fmh_pop_totals* s = pop.dense_summary()) return s->segregating_sites;
  if (pop.dense && pop.dense->ploidy == 2) {
    const vector<uint8_t> mask = pop.dense->mask_for(pop.haplotypes);
    if (mask_count(mask) <= 1 || pop.dense->variants == 0) return 0;
    auto dm = pop.dense->device_matrix();
    return sweep_summaries(*dm, {mask}, FMH_FORMULA_DENSE, 0, dm->variants)[0].segregating_sites;
  }
  // count_segregating_sites_for_haplotypes (3858-3889): no sample-count bound
  return sparse_pop_sweep(*pop.store, pop.store->mask_for(pop.haplotypes, -1)).segregating_sites;
}

optional<double> pi_guards(size_t n_haplotypes, int64_t seq_length) {
  if (n_haplotypes <= 1) return std::nan("");
  if (seq_length < 0) return 0.0;
  if (seq_length == 0) return std::numeric_limits<double>::infinity();
  return std::nullopt;
}

// calculate_pi, stats.rs:4317-4432
double calculate_pi_sparse(const Store& store, const vector<Hap>& haps, int64_t seq_length) {
  if (auto early = pi_guards(haps.size(), seq_length)) return *early;
  int64_t hap_sample_count = 0;
  for (auto& h : haps) hap_sample_count = std::max(hap_sample_count, h.first + 1);
  const int64_t sample_count = std::max(store.first_sample_count(), hap_sample_count);
  const vector<uint8_t> mask = store.mask_for(haps, sample_count);
  // HapMembership.total counts members inside sample_count even beyond the stored columns
  std::set<Hap> members;
  for (auto& h : haps) if (h.first < sample_count) members.insert(h);
  if (members.size() <= 1) return std::nan("");
  const fmh_pop_totals t = sparse_pop_sweep(store, mask);
  const int64_t effective = sat_sub(seq_length, (int64_t)t.uncallable_sites);
  if (effective == 0) return std::nan("");
  return t.pi_sum / (double)effective;
}

// calculate_pi_from_summary[_with_precomputed], stats.rs:1476-1542
double pi_from_summary(const fmh_pop_totals& s, int64_t seq_length, const double* precomputed) {
  if (auto early = pi_guards((size_t)s.haplotype_capacity, seq_length)) return *early;
  const int64_t effective = sat_sub(seq_length, (int64_t)s.uncallable_sites);
  if (effective == 0) return std::nan("");
  return (precomputed ? *precomputed : s.pi_sum) / (double)effective;
}

// calculate_pi_for_population, stats.rs:4599-4614
double calculate_pi_for_population(const Population& pop) {
  const int64_t L = pop.sequence_length;
  if (const fmh_pop_totals* s = pop.dense_summary()) return pi_from_summary(*s, L, nullptr);
  if (pop.dense && pop.dense->ploidy == 2) {  // calculate_pi_dense, stats.rs:4534-4597
    const vector<uint8_t> mask = pop.dense->mask_for(pop.haplotypes);
    if (auto early = pi_guards(mask_count(mask), L)) return *early;
    if (pop.dense->variants == 0) return 0.0 / (double)L;
    auto dm = pop.dense->device_matrix();
    const fmh_pop_totals t = sweep_summaries(*dm, {mask}, FMH_FORMULA_DENSE, 0, dm->variants)[0];
    const int64_t effective = sat_sub(L, (int64_t)t.uncallable_sites);
    if (effective == 0) return std::nan("");
    return t.pi_sum / (double)effective;
  }
  return calculate_pi_sparse(*pop.store, pop.haplotypes, L);
}

bool variants_compatible(const Store& a, const Store& b) {  // stats.rs:3399-3401
  return a.S == b.S && a.positions == b.positions;
}

vector<int64_t> region_rows(const Store& st, int64_t start, int64_t end) {
  vector<int64_t> rows;
  for (int64_t i = 0; i < st.S; ++i) if (st.positions[(size_t)i] >= start && st.positions[(size_t)i] <= end) rows.push_back(i);
  return rows;
}

// Both populations' membership over ONE device matrix.  The reference reads both through pop1's variants when the
// slices are different objects with equal positions (stats.rs:3050-3055).
struct SparseHudson {
  shared_ptr<const Store> store;
  bool swept = false;
  HudsonOut res;
};
SparseHudson hudson_sites_sparse(const Population& p1, const Population& p2, const vector<int64_t>* rows, bool want_sites = true) {
  SparseHudson out;
  out.store = rows ? store_subset(p1.store, *rows) : p1.store;
  const vector<uint8_t> m1 = out.store->mask_for(p1.haplotypes, (int64_t)p1.sample_names.size());
  const vector<uint8_t> m2 = out.store->mask_for(p2.haplotypes, (int64_t)p2.sample_names.size());
  if (out.store->S == 0) return out;
  auto [dm, r0, rc] = out.store->device_rows();
  out.res = sweep_hudson(*dm, m1, m2, FMH_FORMULA_SPARSE, r0, rc, want_sites);
  out.swept = true;
  return out;
}

optional<double> nan_to_none(double x) { return std::isnan(x) ? optional<double>() : optional<double>(x); }

py::list sites_to_py(const Store& store, const HudsonOut& r) {
  py::list out;
  if (!r.have_sites) return out;
  const size_t n = (size_t)store.S;
  for (size_t i = 0; i < n; ++i) {
    HudsonFstSite s{store.positions[i] + 1, nan_to_none(r.fst[i]), nan_to_none(r.dxy[i]), nan_to_none(r.pi1[i]), nan_to_none(r.pi2[i]),
                    (int64_t)r.called[i], (int64_t)r.called[n + i], nan_to_none(r.num[i]), nan_to_none(r.den[i])};
    out.append(py::cast(std::move(s)));
  }
  return out;
}

// aggregate_hudson_components_from_summaries (stats.rs:1554-1623).  Both summaries come from dense matrices: the same matrix -> one
// fused sweep reads it once; two matrices -> the pair is computed from the two populations' per-site count tables (below).
fmh_hudson_totals summary_pair_totals(const Population& p1, const Population& p2) {
  fmh_hudson_totals zero;
  memset(&zero, 0, sizeof zero);
  shared_ptr<Dense> d1 = p1.dense, d2 = p2.dense;
  if (d1 == d2) {
    auto dm = d1->device_matrix();
    if (dm->variants == 0) return zero;
    return sweep_hudson(*dm, d1->mask_for(p1.haplotypes), d2->mask_for(p2.haplotypes), FMH_FORMULA_SUMMARY, 0, dm->variants, false).t;
  }
  // two matrices: the pair from the populations' per-site count tables over the first min(S1, S2) sites (the zip of the two summaries,
  // stats.rs:1562-1566) - no joint matrix is built or uploaded (until round 3 every call copied both matrices side by side on the host)
  const int64_t S = std::min(d1->variants, d2->variants);
  if (S == 0) return zero;
  const Population::SiteCounts &k1 = p1.dense_site_counts(), &k2 = p2.dense_site_counts();
  if (k1.device != k2.device) value_error("populations live on different devices");
  fmh_hudson_totals t;
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_hudson_from_counts(k1.device, (const uint32_t*)k1.called->p, (const uint32_t*)k1.alt->p, mask_count(d1->mask_for(p1.haplotypes)),
                                    (const uint32_t*)k2.called->p, (const uint32_t*)k2.alt->p, mask_count(d2->mask_for(p2.haplotypes)), (size_t)S,
                                    FMH_FORMULA_SUMMARY, (d1->has_missing() || d2->has_missing()) ? 1 : 0, nullptr, &t, nullptr);
  }
  fmh_check(status);
  return t;
}

// calculate_d_xy_hudson, stats.rs:2403-2524
optional<double> calculate_d_xy_hudson(const Population& p1, const Population& p2) {
  if (p1.sequence_length <= 0) vcf_error("InvalidRegion", "Sequence length must be positive for Dxy calculation");
  if (p1.sequence_length != p2.sequence_length) vcf_error("Parse", "Sequence length mismatch in Dxy calculation");
  if (!variants_compatible(*p1.store, *p2.store)) vcf_error("Parse", "Variant slices differ in positions/length for Dxy calculation");
  if (p1.haplotypes.empty() || p2.haplotypes.empty()) return std::nullopt;
  const int64_t L = p1.sequence_length;
  const fmh_pop_totals *s1 = p1.dense_summary(), *s2 = p2.dense_summary();
  if (s1 && s2) {  // dxy_from_summaries, 1637-1662
    const fmh_hudson_totals t = summary_pair_totals(p1, p2);
    const int64_t effective = sat_sub(L, (int64_t)t.dxy_uncallable_sites);
    return effective > 0 ? optional<double>(t.dxy_sum_all / (double)effective) : std::nullopt;
  }
  if (p1.dense && p1.dense == p2.dense && p1.dense->ploidy == 2) {  // calculate_dxy_dense, 2526-2611
    const vector<uint8_t> ma = p1.dense->mask_for(p1.haplotypes), mb = p1.dense->mask_for(p2.haplotypes);
    if (mask_count(ma) == 0 || mask_count(mb) == 0) return std::nullopt;
    if (p1.dense->variants == 0) return 0.0 / (double)L;
    auto dm = p1.dense->device_matrix();
    const fmh_hudson_totals t = sweep_hudson(*dm, ma, mb, FMH_FORMULA_DENSE, 0, dm->variants, false).t;
    const int64_t effective = sat_sub(L, (int64_t)t.site_dxy_skipped);
    return effective > 0 ? optional<double>(t.site_dxy_sum / (double)effective) : std::nullopt;
  }
  const SparseHudson sp = hudson_sites_sparse(p1, p2, nullptr, false);  // sparse fold, 2476-2496
  const double sum_dxy = sp.swept ? sp.res.t.site_dxy_sum : 0.0;
  const int64_t skipped = sp.swept ? (int64_t)sp.res.t.site_dxy_skipped : 0;
  const int64_t effective = sat_sub(L, skipped);
  return effective > 0 ? optional<double>(sum_dxy / (double)effective) : std::nullopt;
}

struct Region { int64_t start, end; };
Region build_region(const py::handle& region) {  // lib.rs:1402-1410
  py::sequence s = py::reinterpret_borrow<py::sequence>(region);
  const int64_t start = to_i64(s[0]), end = to_i64(s[1]);
  if (end < start) value_error("region end must be greater than or equal to region start");
  return {start, end};
}
int64_t region_len(const Region& r) {  // QueryRegion::len, process.rs:573-584
  if (r.start > r.end) return 0;
  const int64_t a = std::max<int64_t>(r.start, 0);
  const int64_t b = r.end < a ? a : std::max<int64_t>(r.end + 1, a);
  return b > a ? b - a : 0;
}

// calculate_hudson_fst_for_pair_core, stats.rs:3435-3599
std::pair<HudsonFstResult, py::list> hudson_core(const Population& p1, const Population& p2, const Region* region) {
  if (p1.sequence_length <= 0) vcf_error("InvalidRegion", "Sequence length must be positive for Hudson FST calculation.");
  if (p1.sequence_length != p2.sequence_length) vcf_error("Parse", "Sequence length mismatch between population contexts for Hudson FST calculation.");
  if (!variants_compatible(*p1.store, *p2.store)) vcf_error("Parse", "Variant slices differ in positions/length.");
  const int64_t L = p1.sequence_length;
  const fmh_pop_totals *s1 = p1.dense_summary(), *s2 = p2.dense_summary();
  optional<fmh_hudson_totals> summary_totals;
  shared_ptr<Dense> dense_shared = (p1.dense && p1.dense == p2.dense && p1.dense->ploidy == 2) ? p1.dense : nullptr;
  py::list sites;
  double num_sum = 0.0, den_sum = 0.0;
  if (region) {
    const vector<int64_t> rows = region_rows(*p1.store, region->start, region->end);
    const SparseHudson sp = hudson_sites_sparse(p1, p2, &rows);
    if (sp.swept) { sites = sites_to_py(*sp.store, sp.res); num_sum = sp.res.t.site_num_sum; den_sum = sp.res.t.site_den_sum; }
  } else if (s1 && s2) {
    summary_totals = summary_pair_totals(p1, p2);
    num_sum = summary_totals->numerator_sum; den_sum = summary_totals->denominator_sum;
  } else if (dense_shared) {
    if (p1.store->S != 0) {
      auto dm = dense_shared->device_matrix();
      const HudsonOut r = sweep_hudson(*dm, dense_shared->mask_for(p1.haplotypes), dense_shared->mask_for(p2.haplotypes), FMH_FORMULA_DENSE, 0,
                                       dm->variants, true);
      num_sum = r.t.site_num_sum; den_sum = r.t.site_den_sum;
      sites = sites_to_py(*p1.store, r);
    }
  } else if (p1.store->S != 0) {
    const SparseHudson sp = hudson_sites_sparse(p1, p2, nullptr);
    sites = sites_to_py(*sp.store, sp.res);
    num_sum = sp.res.t.site_num_sum; den_sum = sp.res.t.site_den_sum;
  }
  HudsonFstResult out;
  if (den_sum > kFstEpsilon) out.fst = num_sum / den_sum;
  double pi1_raw, pi2_raw;
  if (summary_totals) {
    pi1_raw = pi_from_summary(*s1, L, &summary_totals->pi1_sum);
    pi2_raw = pi_from_summary(*s2, L, &summary_totals->pi2_sum);
    if (!p1.haplotypes.empty() && !p2.haplotypes.empty()) {
      const int64_t effective = sat_sub(L, (int64_t)summary_totals->dxy_uncallable_sites);
      if (effective > 0) out.d_xy = summary_totals->dxy_sum_all / (double)effective;
    }
  } else {
    pi1_raw = calculate_pi_for_population(p1);
    pi2_raw = calculate_pi_for_population(p2);
    out.d_xy = calculate_d_xy_hudson(p1, p2);
  }
  if (std::isfinite(pi1_raw)) out.pi_pop1 = pi1_raw;
  if (std::isfinite(pi2_raw)) out.pi_pop2 = pi2_raw;
  if (out.pi_pop1 && out.pi_pop2) out.pi_xy_avg = 0.5 * (*out.pi_pop1 + *out.pi_pop2);
  population_label(p1.id, &out.population1_label, &out.population1_haplotype_group);
  population_label(p2.id, &out.population2_label, &out.population2_haplotype_group);
  return {out, sites};
}

// ---------------------------------------------------------------------------------------------------------------
// module-level functions (lib.rs:1555-1778, 2190-2225)
// ---------------------------------------------------------------------------------------------------------------
// count_segregating_sites, stats.rs:3808-3829: every called allele of every sample
uint64_t segregating_sites(const py::object& variants) {
  auto store = store_from_python(variants);
  if (store->S == 0) return 0;
  return sparse_pop_sweep(*store, vector<uint8_t>((size_t)(store->N * store->P), 1)).segregating_sites;
}

double nucleotide_diversity(const py::object& variants, const py::object& haplotypes, const py::object& sequence_length) {
  const int64_t L = positive_length(sequence_length);
  auto store = store_from_python(variants);
  return calculate_pi_sparse(*store, parse_haplotypes(haplotypes), L);
}

// watterson_theta_py (lib.rs:1593-1613) -> calculate_watterson_theta (stats.rs:4243-4307): scalar host arithmetic
double watterson_theta(const py::object& seg, const py::object& samples, const py::object& sequence_length) {
  const int64_t s = to_i64(seg), n = to_i64(samples), L = to_i64(sequence_length);
  if (s < 0 || n < 0) raise(PyExc_OverflowError, "can't convert negative int to unsigned");
  if (n <= 1) value_error("sample_count must be greater than 1 for Watterson's theta");
  if (L <= 0) value_error("sequence_length must be a positive integer");
  double h = 0.0;  // harmonic, stats.rs:4234-4240
  for (int64_t k = 1; k <= n - 1; ++k) h += 1.0 / (double)k;
  if (h > 0.0) return (double)s / h / (double)L;
  return s == 0 ? std::nan("") : std::numeric_limits<double>::infinity();
}

// pairwise_differences_py (lib.rs:1620-1636) -> calculate_pairwise_differences (stats.rs:4106-4231).  The all-vs-all
// allele comparison of every sample pair is a Gram product over sites on the GPU; ploidy detection and the
// comparable-site arithmetic are host scalars.
py::list pairwise_differences(const py::object& variants, const py::object& sample_count, const py::object& sequence_length) {
  const int64_t L = positive_length(sequence_length);
  const int64_t n = to_i64(sample_count);
  if (n < 0) raise(PyExc_OverflowError, "can't convert negative int to unsigned");
  auto store = store_from_python(variants);
  const int64_t S = store->S, N = S ? store->N : 0;
  // haplotype_counts: length of the first Some genotype of each sample (stats.rs:4124-4137)
  vector<int64_t> hap_counts((size_t)n, 0);
  const int64_t m = std::min(n, N);
  for (int64_t idx = 0; idx < m; ++idx)
    for (int64_t s = 0; s < S; ++s) {
      if (idx >= store->num_samples[(size_t)s]) continue;
      const size_t base = ((size_t)s * (size_t)store->N + (size_t)idx) * (size_t)store->P;
      if (!store->called[base]) continue;
      int64_t len = 0;
      for (int64_t k = 0; k < store->P; ++k) len += store->called[base + (size_t)k];
      hap_counts[(size_t)idx] = len;
      break;
    }
  vector<uint64_t> diff, both;
  if (S && m >= 2) {
    auto dm = store->device_matrix();
    DevBuf d_diff(dm->device, 8 * (size_t)(m * m)), d_both(dm->device, 8 * (size_t)(m * m));
    fmh_check(fmh_device_zero(dm->device, d_diff.p, 8 * (size_t)(m * m), nullptr));
    fmh_check(fmh_device_zero(dm->device, d_both.p, 8 * (size_t)(m * m), nullptr));
    int status;
    {
      py::gil_scoped_release nogil;
      status = fmh_pairwise_differences(dm->h, (size_t)m, (unsigned long long*)d_diff.p, (unsigned long long*)d_both.p, nullptr);
    }
    fmh_check(status);
    diff = d_diff.fetch<uint64_t>((size_t)(m * m));
    both = d_both.fetch<uint64_t>((size_t)(m * m));
  }
  py::list out;
  const py::int_ zero_int(0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j) {
      const int64_t hi = hap_counts[(size_t)i], hj = hap_counts[(size_t)j];
      if (hi == 0 || hj == 0) { out.append(py::cast(PairwiseDifference{i, j, zero_int, zero_int})); continue; }
      const py::int_ product(hi * hj);
      const uint64_t d = diff[(size_t)(i * m + j)];
      const int64_t missing_sites = S - (int64_t)both[(size_t)(i * m + j)];
      py::object comparable = py::int_(L) * product - py::int_(missing_sites) * product;
      if (comparable < zero_int) comparable = zero_int;
      out.append(py::cast(PairwiseDifference{i, j, py::int_(d), comparable}));
    }
  return out;
}

// per_site_diversity_py (lib.rs:1644-1665) -> calculate_per_site_diversity (stats.rs:4628-4806)
py::list per_site_diversity(const py::object& variants, const py::object& haplotypes, const py::object& region) {
  auto store = store_from_python(variants);
  const vector<Hap> haps = parse_haplotypes(haplotypes);
  if (haps.size() < 2) value_error("at least two haplotypes are required for diversity calculations");
  Region reg;
  if (!region.is_none()) reg = build_region(region);
  else {
    if (store->S == 0) value_error("region must be provided when no variants are supplied");
    reg = {*std::min_element(store->positions.begin(), store->positions.end()), *std::max_element(store->positions.begin(), store->positions.end())};
  }
  py::list out;
  if (region_len(reg) <= 0) return out;
  const vector<int64_t> rows = region_rows(*store, reg.start, reg.end);
  if (rows.empty()) return out;
  const vector<uint8_t> mask = store->mask_for(haps, store->first_sample_count());  // membership from the FIRST variant's sample count
  auto sub = store_subset(store, rows);
  auto [dm, r0, rc] = sub->device_rows();
  const shared_ptr<Groups> gp = groups_for(*dm, {mask});
  Groups& g = *gp;
  DevBuf d_pi(dm->device, 8 * rc), d_th(dm->device, 8 * rc);
  fmh_pop_totals totals;
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_diversity_sites(dm->h, g.h, r0, rc, (double*)d_pi.p, (double*)d_th.p, nullptr, nullptr, &totals, nullptr);
  }
  fmh_check(status);
  const vector<double> pi = d_pi.fetch<double>(rc), th = d_th.fetch<double>(rc);
  for (size_t i = 0; i < rc; ++i) out.append(py::cast(DiversitySite{sub->positions[i] + 1, pi[i], th[i]}));
  return out;
}

// process.rs:1198-1241
std::map<string, int64_t> map_sample_names_to_indices(const vector<string>& names) {
  std::map<string, int64_t> exact;
  std::map<string, int64_t> alias;  // -1 = ambiguous
  vector<string> alias_order;
  for (size_t i = 0; i < names.size(); ++i) {
    exact[names[i]] = (int64_t)i;
    const size_t us = names[i].rfind('_');
    if (us == string::npos) continue;
    const string suffix = names[i].substr(us + 1);
    auto it = alias.find(suffix);
    if (it == alias.end()) { alias[suffix] = (int64_t)i; alias_order.push_back(suffix); }
    else if (it->second != (int64_t)i) it->second = -1;
  }
  for (auto& a : alias_order) {
    const int64_t target = alias[a];
    if (target >= 0 && !exact.count(a)) exact[a] = target;
  }
  return exact;
}
string normalize_sample_name_for_lookup(const string& n) {  // process.rs:1192-1196
  if (n.size() >= 2 && (n.compare(n.size() - 2, 2, "_L") == 0 || n.compare(n.size() - 2, 2, "_R") == 0)) return n.substr(0, n.size() - 2);
  return n;
}

// lib.rs:1485-1505; insertion order kept (Python dict order)
vector<std::pair<string, std::pair<int, int>>> extract_sample_group_map(const py::handle& obj) {
  if (!py::isinstance<py::dict>(obj)) value_error("sample_to_group must be a dict mapping sample -> (left, right)");
  vector<std::pair<string, std::pair<int, int>>> out;
  for (auto kv : py::reinterpret_borrow<py::dict>(obj)) {
    py::object left, right;
    try {
      left = kv.second[py::int_(0)];
      right = kv.second[py::int_(1)];
    } catch (py::error_already_set&) {
      value_error("group tuples must contain two entries");
    }
    const string key = py::cast<string>(py::str(kv.first));
    const std::pair<int, int> val{extract_u8(left), extract_u8(right)};
    bool replaced = false;
    for (auto& e : out) if (e.first == key) { e.second = val; replaced = true; }
    if (!replaced) out.push_back({key, val});
  }
  return out;
}

// wc_fst_py (lib.rs:1750-1770) -> calculate_fst_wc_haplotype_groups (stats.rs:675-806)
WcFstResult wc_fst(const py::object& variants, const py::object& sample_names_obj, const py::object& sample_to_group, const py::object& region) {
  const vector<string> sample_names = to_string_list(sample_names_obj);
  if (sample_names.empty()) value_error("sample_names must contain at least one sample");
  auto store = store_from_python(variants);
  const auto group_map = extract_sample_group_map(sample_to_group);
  const Region reg = build_region(region);
  // map_samples_to_haplotype_groups (1036-1052) + SubpopulationMembership::from_map (1104-1150)
  const auto idx_of = map_sample_names_to_indices(sample_names);
  std::map<Hap, string> hap_to_group;
  for (auto& kv : group_map) {
    auto it = idx_of.find(normalize_sample_name_for_lookup(kv.first));
    if (it == idx_of.end()) continue;
    hap_to_group[{it->second, kLeft}] = std::to_string(kv.second.first);
    hap_to_group[{it->second, kRight}] = std::to_string(kv.second.second);
  }
  std::set<string> label_set;
  for (auto& kv : hap_to_group) label_set.insert(kv.second);
  const vector<string> labels(label_set.begin(), label_set.end());
  const size_t G = labels.size();
  vector<string> keys;
  for (size_t i = 0; i < G; ++i) for (size_t j = i + 1; j < G; ++j) keys.push_back(labels[i] + "_vs_" + labels[j]);
  WcFstResult result;
  result.fst_type = "haplotype_groups";
  const vector<int64_t> rows = region_rows(*store, reg.start, reg.end);
  if (rows.empty()) { result.overall_fst = insufficient(0); return result; }  // stats.rs:2152-2159
  auto sub = store_subset(store, rows);
  const int64_t N = sub->N, P = sub->P;
  vector<vector<uint8_t>> masks(std::max<size_t>(G, 1), vector<uint8_t>((size_t)(N * P), 0));
  for (auto& kv : hap_to_group) {
    const int64_t sample_idx = kv.first.first;
    const int side = kv.first.second;
    if (sample_idx >= (int64_t)sample_names.size() || sample_idx >= N || side >= P) continue;
    const size_t gi = (size_t)(std::find(labels.begin(), labels.end(), kv.second) - labels.begin());
    masks[gi][(size_t)(sample_idx * P + side)] = 1;
  }
  auto [dm, r0, rc] = sub->device_rows();
  if (G < 2) {
    // fewer than two groups: every site with any called allele is NoInterPopulationVariance (0, 0), sites without any call
    // are InsufficientData (stats.rs:1925-1930, 1987-2003).  One summary sweep over all columns supplies "any call".
    vector<vector<uint8_t>> gm{vector<uint8_t>((size_t)(N * P), 1)};
    if (G == 1) gm.push_back(masks[0]);
    vector<uint32_t> called;
    sweep_summaries(*dm, gm, FMH_FORMULA_SPARSE, r0, rc, nullptr, &called);
    size_t n_inf = 0;
    for (size_t i = 0; i < rc; ++i) {
      WcFstSite s;
      s.position = sub->positions[i] + 1;
      s.variance_components_a = 0.0; s.variance_components_b = 0.0;
      if (called[i] == 0) s.overall_fst = insufficient(1);
      else {
        s.overall_fst = classify(0.0, 0.0, 1);
        ++n_inf;
        if (G == 1 && called[rc + i] > 0) s.population_sizes[py::str(labels[0])] = py::int_(called[rc + i]);
      }
      result.site_fst.append(py::cast(std::move(s)));
    }
    result.overall_fst = n_inf == 0 ? insufficient(rc) : classify(0.0, 0.0, n_inf);
    return result;
  }
  const WcOut w = sweep_wc(*dm, masks, r0, rc);
  bool any_site_with_pairs = false;
  vector<size_t> attempted(keys.size(), 0);
  for (size_t i = 0; i < rc; ++i) {
    WcFstSite s;
    s.position = sub->positions[i] + 1;
    if (w.state[i] == 3) {
      s.overall_fst = insufficient(1);
      s.variance_components_a = 0.0; s.variance_components_b = 0.0;
      result.site_fst.append(py::cast(std::move(s)));
      continue;
    }
    any_site_with_pairs = true;
    s.overall_fst = classify(w.a[i], w.b[i], 1);
    s.variance_components_a = w.a[i]; s.variance_components_b = w.b[i];
    for (size_t k = 0; k < keys.size(); ++k) {
      const size_t at = (k + 1) * rc + i;
      const py::str key(keys[k]);
      if (w.state[at] == 3) { s.pairwise_fst[key] = py::cast(insufficient(1)); s.pairwise_variance_components[key] = py::make_tuple(0.0, 0.0); }
      else { s.pairwise_fst[key] = py::cast(classify(w.a[at], w.b[at], 1)); s.pairwise_variance_components[key] = py::make_tuple(w.a[at], w.b[at]); }
      ++attempted[k];
    }
    for (size_t g = 0; g < G; ++g) if (w.group_called[g * rc + i] > 0) s.population_sizes[py::str(labels[g])] = py::int_(w.group_called[g * rc + i]);
    result.site_fst.append(py::cast(std::move(s)));
  }
  // calculate_overall_fst_wc, stats.rs:2145-2374 (sums come from the device sweep)
  result.overall_fst = w.informative[0] == 0 ? insufficient(rc) : classify(w.sum_a[0], w.sum_b[0], (size_t)w.informative[0]);
  if (any_site_with_pairs) {
    for (size_t k = 0; k < keys.size(); ++k) {
      const py::str key(keys[k]);
      const size_t n_inf = (size_t)w.informative[k + 1];
      if (n_inf > 0) { result.pairwise_fst[key] = py::cast(classify(w.sum_a[k + 1], w.sum_b[k + 1], n_inf)); result.pairwise_variance_components[key] = py::make_tuple(w.sum_a[k + 1], w.sum_b[k + 1]); }
      else { result.pairwise_fst[key] = py::cast(insufficient(attempted[k])); result.pairwise_variance_components[key] = py::make_tuple(0.0, 0.0); }
    }
  }
  return result;
}

// lib.rs:1527-1549
optional<vector<std::pair<int64_t, int64_t>>> extract_interval_list(const py::object& obj) {
  if (obj.is_none()) return std::nullopt;
  vector<std::pair<int64_t, int64_t>> out;
  for (py::handle entry : obj) {
    int64_t start, end;
    try {
      start = to_i64(entry[py::int_(0)]);
      end = to_i64(entry[py::int_(1)]);
    } catch (py::error_already_set&) {
      value_error("intervals must be (start, end)");
    }
    if (end < start) value_error("interval end must be greater than or equal to start");
    out.push_back({start, end});
  }
  return out;
}

// adjusted_sequence_length_py (lib.rs:2196-2215) -> calculate_adjusted_sequence_length (stats.rs:3644-3775): interval arithmetic only
int64_t adjusted_sequence_length(int64_t start, int64_t end, const py::object& allow_obj, const py::object& mask_obj) {
  if (end < start) value_error("end must be greater than or equal to start");
  const auto allow = extract_interval_list(allow_obj), mask = extract_interval_list(mask_obj);
  typedef std::pair<int64_t, int64_t> Iv;
  const int64_t a = std::max<int64_t>(start, 1), b = end >= a ? end : a;
  const int64_t r0 = a - 1, r1 = b;  // region as 0-based half-open (process.rs:193-206)
  vector<Iv> allowed;
  if (allow) {
    for (auto& iv : *allow) {
      const int64_t lo = std::max(r0, iv.first), hi = std::min(r1, iv.second);
      if (lo < hi) allowed.push_back({lo + 1, hi});
    }
  } else {
    allowed.push_back({start, end});
  }
  if (mask) {
    vector<Iv> masks, out;
    for (auto& iv : *mask) masks.push_back({iv.first + 1, iv.second});
    for (auto& al : allowed) {  // subtract_regions, stats.rs:3739-3775
      vector<Iv> parts{al};
      for (auto& m : masks) {
        vector<Iv> nxt;
        for (auto& p : parts) {
          if (m.second < p.first || m.first > p.second) { nxt.push_back(p); continue; }
          if (m.first > p.first && m.first - 1 >= p.first) nxt.push_back({p.first, m.first - 1});
          if (m.second < p.second && m.second + 1 <= p.second) nxt.push_back({m.second + 1, p.second});
        }
        parts = nxt;
        if (parts.empty()) break;
      }
      out.insert(out.end(), parts.begin(), parts.end());
    }
    allowed = out;
  }
  int64_t total = 0;
  for (auto& iv : allowed) {
    const int64_t lo = std::max<int64_t>(iv.first, 1), hi = iv.second >= lo ? iv.second : lo;
    total += std::max<int64_t>(hi - (lo - 1), 0);
  }
  return total;
}

// calculate_inversion_allele_frequency, stats.rs:3778-3805 (host scalar)
optional<double> inversion_allele_frequency(const py::object& sample_map) {
  int64_t ones = 0, total = 0;
  for (auto& kv : extract_sample_group_map(sample_map))
    for (int allele : {kv.second.first, kv.second.second})
      if (allele == 0 || allele == 1) { ++total; ones += allele; }
  return total > 0 ? optional<double>((double)ones / (double)total) : std::nullopt;
}

// ---- what the device statistics below share: the rows they run over, the samples and haplotypes in play, their argument rules ---------------
#include "pymodule_rows.inc"

#include "pymodule_ld.inc"
#include "pymodule_sfs.inc"
#include "pymodule_hap.inc"
#include "pymodule_ehh.inc"
#include "pymodule_fstat.inc"
#include "pymodule_kinship.inc"
#include "pymodule_qc.inc"
#include "pymodule_assoc.inc"
#include "pymodule_logistic.inc"
#include "pymodule_score.inc"
#include "pymodule_segments.inc"
#include "pymodule_roh.inc"
#include "pymodule_ibd.inc"
#include "pymodule_clump.inc"
#include "pymodule_ldscore.inc"
#include "pymodule_grm.inc"
#include "pymodule_lmm.inc"
#include "pymodule_admix.inc"

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "ferromic drop-in: per-site diversity / FST statistics on MI355X (C++ host over libferromic_hip.so)";

  py::class_<FstEstimate>(m, "FstEstimate")
      .def(py::init([](string state, py::object value, py::object sum_a, py::object sum_b, py::object sites) {
             return FstEstimate{std::move(state), std::move(value), std::move(sum_a), std::move(sum_b), std::move(sites)};
           }), py::arg("state"), py::arg("value"), py::arg("sum_a"), py::arg("sum_b"), py::arg("sites"))
      .def_readonly("state", &FstEstimate::state)
      .def_readonly("value", &FstEstimate::value)
      .def_readonly("sum_a", &FstEstimate::sum_a)
      .def_readonly("sum_b", &FstEstimate::sum_b)
      .def_readonly("sites", &FstEstimate::sites)
      .def("components", &FstEstimate::components)
      .def("__repr__", &FstEstimate::repr);

  py::class_<PairwiseDifference>(m, "PairwiseDifference")
      .def(py::init([](int64_t i, int64_t j, py::object d, py::object c) { return PairwiseDifference{i, j, std::move(d), std::move(c)}; }),
           py::arg("sample_i"), py::arg("sample_j"), py::arg("differences"), py::arg("comparable_sites"))
      .def_readonly("sample_i", &PairwiseDifference::sample_i)
      .def_readonly("sample_j", &PairwiseDifference::sample_j)
      .def_readonly("differences", &PairwiseDifference::differences)
      .def_readonly("comparable_sites", &PairwiseDifference::comparable_sites)
      .def("__repr__", &PairwiseDifference::repr);

  bind_pca(m);

  py::class_<DiversitySite>(m, "DiversitySite")
      .def(py::init([](int64_t p, double pi, double th) { return DiversitySite{p, pi, th}; }), py::arg("position"), py::arg("pi"),
           py::arg("watterson_theta"))
      .def_readonly("position", &DiversitySite::position)
      .def_readonly("pi", &DiversitySite::pi)
      .def_readonly("watterson_theta", &DiversitySite::watterson_theta)
      .def("__repr__", &DiversitySite::repr);

  py::class_<HudsonDxyResult>(m, "HudsonDxyResult")
      .def(py::init([](optional<double> d) { return HudsonDxyResult{d}; }), py::arg("d_xy"))
      .def_readonly("d_xy", &HudsonDxyResult::d_xy)
      .def("__repr__", &HudsonDxyResult::repr);

  py::class_<HudsonFstSite>(m, "HudsonFstSite")
      .def(py::init([](int64_t position, optional<double> fst, optional<double> d_xy, optional<double> pi1, optional<double> pi2, int64_t n1,
                       int64_t n2, optional<double> num, optional<double> den) {
             return HudsonFstSite{position, fst, d_xy, pi1, pi2, n1, n2, num, den};
           }))
      .def_readonly("position", &HudsonFstSite::position)
      .def_readonly("fst", &HudsonFstSite::fst)
      .def_readonly("d_xy", &HudsonFstSite::d_xy)
      .def_readonly("pi_pop1", &HudsonFstSite::pi_pop1)
      .def_readonly("pi_pop2", &HudsonFstSite::pi_pop2)
      .def_readonly("n1_called", &HudsonFstSite::n1_called)
      .def_readonly("n2_called", &HudsonFstSite::n2_called)
      .def_readonly("numerator_component", &HudsonFstSite::numerator_component)
      .def_readonly("denominator_component", &HudsonFstSite::denominator_component)
      .def("__repr__", &HudsonFstSite::repr);

  py::class_<HudsonFstResult>(m, "HudsonFstResult")
      .def_readonly("fst", &HudsonFstResult::fst)
      .def_readonly("d_xy", &HudsonFstResult::d_xy)
      .def_readonly("pi_pop1", &HudsonFstResult::pi_pop1)
      .def_readonly("pi_pop2", &HudsonFstResult::pi_pop2)
      .def_readonly("pi_xy_avg", &HudsonFstResult::pi_xy_avg)
      .def_readonly("population1_label", &HudsonFstResult::population1_label)
      .def_readonly("population1_haplotype_group", &HudsonFstResult::population1_haplotype_group)
      .def_readonly("population2_label", &HudsonFstResult::population2_label)
      .def_readonly("population2_haplotype_group", &HudsonFstResult::population2_haplotype_group)
      .def("__repr__", &HudsonFstResult::repr);

  py::class_<WcFstSite>(m, "WcFstSite")
      .def_readonly("position", &WcFstSite::position)
      .def_readonly("overall_fst", &WcFstSite::overall_fst)
      .def_readonly("pairwise_fst", &WcFstSite::pairwise_fst)
      .def_readonly("variance_components_a", &WcFstSite::variance_components_a)
      .def_readonly("variance_components_b", &WcFstSite::variance_components_b)
      .def_readonly("population_sizes", &WcFstSite::population_sizes)
      .def_readonly("pairwise_variance_components", &WcFstSite::pairwise_variance_components)
      .def("variance_components", [](const WcFstSite& s) { return py::make_tuple(s.variance_components_a, s.variance_components_b); })
      .def("__repr__", &WcFstSite::repr);

  py::class_<WcFstResult>(m, "WcFstResult")
      .def_readonly("overall_fst", &WcFstResult::overall_fst)
      .def_readonly("pairwise_fst", &WcFstResult::pairwise_fst)
      .def_readonly("pairwise_variance_components", &WcFstResult::pairwise_variance_components)
      .def_readonly("site_fst", &WcFstResult::site_fst)
      .def_readonly("fst_type", &WcFstResult::fst_type)
      .def("__repr__", &WcFstResult::repr);

  py::class_<Population, shared_ptr<Population>> population(m, "Population");
  population
      .def(py::init([](const py::object& id, const py::object& variants, const py::object& haplotypes, const py::object& sequence_length,
                       const py::object& sample_names) {
             const int64_t L = positive_length(sequence_length);
             return make_population(parse_population_id(id), store_from_python(variants), parse_haplotypes(haplotypes), to_string_list(sample_names), L,
                                    nullptr);
           }), py::arg("id"), py::arg("variants"), py::arg("haplotypes"), py::arg("sequence_length"), py::arg("sample_names") = py::none())
      .def_static("from_numpy",
                  [](const py::object& id, const py::object& genotypes, const py::object& positions, const py::object& haplotypes,
                     const py::object& sequence_length, const py::object& sample_names) {
                    const int64_t L = positive_length(sequence_length);
                    const PopId pid = parse_population_id(id);
                    vector<Hap> haps = parse_haplotypes(haplotypes);
                    auto conv = convert_numeric_array(genotypes, positions);
                    return make_population(pid, conv.first, std::move(haps), to_string_list(sample_names), L, conv.second);
                  },
                  py::arg("id"), py::arg("genotypes"), py::arg("positions"), py::arg("haplotypes"), py::arg("sequence_length"),
                  py::arg("sample_names") = py::none())
      // clone_with_haplotypes, lib.rs:761-775: variants and dense matrix are shared, the summary is not
      .def("with_haplotypes",
           [](const Population& self, const py::object& id, const py::object& haplotypes) {
             return make_population(parse_population_id(id), self.store, parse_haplotypes(haplotypes), self.sample_names, self.sequence_length, self.dense);
           },
           py::arg("id"), py::arg("haplotypes"))
      .def("segregating_sites", [](const Population& self) { return count_segregating_sites_for_population(self); })
      .def("nucleotide_diversity", [](const Population& self) { return calculate_pi_for_population(self); })
      .def("ld_r2", &population_ld_r2, py::arg("max_sites_apart"))
      .def("ld_prune", &population_ld_prune, py::arg("window_sites"), py::arg("r2_threshold"))
      .def("kinship", &population_kinship, py::arg("sites") = py::none())
      .def("genotype_qc", &population_genotype_qc, py::arg("sites") = py::none(), py::arg("hwe") = true, py::arg("inbreeding") = true)
      .def("site_frequency_spectrum", &population_sfs, py::arg("windows") = py::none())
      .def("garud_h", &population_garud_h, py::arg("windows") = py::none(), py::arg("size") = py::none(), py::arg("step") = py::none(),
           py::arg("partition") = false)
      .def_property_readonly("id", [](const Population& p) -> py::object { return p.id.is_group ? py::object(py::int_(p.id.group)) : py::object(py::str(p.id.name)); })
      .def_property_readonly("haplotype_group", [](const Population& p) -> py::object { return p.id.is_group ? py::object(py::int_(p.id.group)) : py::object(py::none()); })
      .def_property_readonly("label", [](const Population& p) -> py::object { return p.id.is_group ? py::object(py::none()) : py::object(py::str(p.id.name)); })
      .def_property_readonly("sequence_length", [](const Population& p) { return p.sequence_length; })
      .def_property_readonly("variant_count", [](const Population& p) { return p.store->S; })
      .def_property_readonly("sample_names", [](const Population& p) { return p.sample_names; })
      .def_property_readonly("haplotypes", [](const Population& p) {
        py::list out;
        for (auto& h : p.haplotypes) out.append(py::make_tuple(h.first, h.second));
        return out;
      })
      .def("__repr__", &Population::repr);

  m.def("segregating_sites", &segregating_sites, py::arg("variants"));
  m.def("nucleotide_diversity", &nucleotide_diversity, py::arg("variants"), py::arg("haplotypes"), py::arg("sequence_length"));
  m.def("watterson_theta", &watterson_theta, py::arg("segregating_sites"), py::arg("sample_count"), py::arg("sequence_length"));
  m.def("pairwise_differences", &pairwise_differences, py::arg("variants"), py::arg("sample_count"), py::arg("sequence_length"));
  m.def("per_site_diversity", &per_site_diversity, py::arg("variants"), py::arg("haplotypes"), py::arg("region") = py::none());
  bind_ld(m);
  bind_sfs(m);
  bind_hap(m);
  bind_ehh(m, population);
  bind_fstat(m);
  bind_kinship(m);
  bind_qc(m);
  bind_assoc(m, population);
  bind_logistic(m, population);
  bind_score(m, population);
  bind_roh(m, population);
  bind_ibd(m, population);
  bind_clump(m, population);
  bind_ldscore(m, population);
  bind_grm(m, population);
  bind_lmm(m, population);
  bind_admix(m, population);
  m.def("hudson_dxy", [](const py::object& a, const py::object& b) {
    auto p1 = coerce_population(a), p2 = coerce_population(b);
    return HudsonDxyResult{calculate_d_xy_hudson(*p1, *p2)};
  }, py::arg("population1"), py::arg("population2"));
  m.def("hudson_fst", [](const py::object& a, const py::object& b) {
    auto p1 = coerce_population(a), p2 = coerce_population(b);
    return hudson_core(*p1, *p2, nullptr).first;
  }, py::arg("population1"), py::arg("population2"));
  // calculate_hudson_fst_per_site, stats.rs:3021-3058: incompatible variants -> []
  m.def("hudson_fst_sites", [](const py::object& a, const py::object& b, const py::object& region) -> py::list {
    const Region reg = build_region(region);
    auto p1 = coerce_population(a), p2 = coerce_population(b);
    if (!variants_compatible(*p1->store, *p2->store)) return py::list();
    const vector<int64_t> rows = region_rows(*p1->store, reg.start, reg.end);
    const SparseHudson sp = hudson_sites_sparse(*p1, *p2, &rows);
    return sp.swept ? sites_to_py(*sp.store, sp.res) : py::list();
  }, py::arg("population1"), py::arg("population2"), py::arg("region"));
  m.def("hudson_fst_with_sites", [](const py::object& a, const py::object& b, const py::object& region) {
    const Region reg = build_region(region);
    auto p1 = coerce_population(a), p2 = coerce_population(b);
    auto res = hudson_core(*p1, *p2, &reg);
    return py::make_tuple(res.first, res.second);
  }, py::arg("population1"), py::arg("population2"), py::arg("region"));
  m.def("wc_fst", &wc_fst, py::arg("variants"), py::arg("sample_names"), py::arg("sample_to_group"), py::arg("region"));
  m.def("wc_fst_components", [](const FstEstimate& e) { return e.components(); }, py::arg("estimate"));
  m.def("adjusted_sequence_length", &adjusted_sequence_length, py::arg("start"), py::arg("end"), py::arg("allow") = py::none(),
        py::arg("mask") = py::none());
  m.def("inversion_allele_frequency", &inversion_allele_frequency, py::arg("sample_map"));
  // device selection (an addition: the reference is CPU-only).  New matrices go to this GPU; FERROMIC_HIP_DEVICES sets the default.
  m.def("set_device", [](int device) {
    int n = 0;
    fmh_check(fmh_device_count(&n));
    if (device < 0 || device >= n) value_error("device " + std::to_string(device) + " out of range (0.." + std::to_string(n - 1) + ")");
    g_device.store(device);
  }, py::arg("device"));
  m.def("get_device", []() { return current_device(); });
  // the multi-chromosome driver is not wired up yet: per_chromosome_pca and _combine_pca_results are its two halves
  m.def("global_pca", [](py::args, py::kwargs) -> py::object { pca_unavailable(); });
}
