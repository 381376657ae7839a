// pymodule_score.inc — ferromic.polygenic_score, Population.polygenic_score and the PolygenicScore result (included inside
// pymodule_stats.inc's namespace, after pymodule_assoc.inc whose sample rules and array helpers it reuses).  An addition to the reference's
// surface: it has no scores; the definition is include/ferromic_hip.h's (fmh_score_exponents, fmh_score_values, fmh_score_sums,
// fmh_score_stats).  The exact sums come from the device, row chunk by row chunk, and are added in i64; the scores are computed from the
// totals on the host by the library, once; the GIL is released around the C calls.

struct PolygenicScore {
  size_t n = 0, K = 0;
  int mode = FMH_SCORE_MEAN;
  uint64_t rows_used = 0;
  vector<double> score;                  // [n][K]
  vector<uint64_t> n_called, dosage_sum; // [n]
  vector<int32_t> exponents;             // [K]
  vector<int64_t> positions;             // [rows in play] (empty when built from sums without them)

  py::array_t<double> table(bool average) const {
    py::array_t<double> out({(py::ssize_t)n, (py::ssize_t)K});
    double* dst = out.mutable_data();
    const double alleles = (double)(2 * rows_used);
    for (size_t i = 0; i < score.size(); ++i) dst[i] = average ? score[i] / alleles : score[i];
    return out;
  }
  const char* mode_name() const { return mode == FMH_SCORE_MEAN ? "mean" : mode == FMH_SCORE_CENTER ? "center" : "zero"; }
  string repr() const {
    return "PolygenicScore(samples=" + std::to_string(n) + ", columns=" + std::to_string(K) + ", rows_used=" + std::to_string(rows_used) + ", mode=" +
           mode_name() + ")";
  }
};

int score_mode_arg(const string& missing, bool center) {
  if (missing != "mean" && missing != "zero") value_error("missing must be \"mean\" or \"zero\", got \"" + missing + "\"");
  if (center && missing == "zero") value_error("center=True already lets a missing genotype contribute 0: it does not combine with missing=\"zero\"");
  return center ? FMH_SCORE_CENTER : missing == "zero" ? FMH_SCORE_ZERO : FMH_SCORE_MEAN;
}

// what the weights argument holds, checked against the rows in play; every argument error before any device use
struct ScoreWeights {
  size_t rows = 0, K = 0;
  vector<double> w;           // [rows][K]
  vector<int32_t> exponents;  // [K]
  vector<uint8_t> keep;       // [rows]: some weight of the row is not zero
};

ScoreWeights score_weights_arg(const py::object& weights, size_t rows) {
  auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(weights);
  if (!arr || (arr.ndim() != 1 && arr.ndim() != 2)) value_error("weights must be a numeric array [rows] or [rows][K]");
  if ((size_t)arr.shape(0) != rows) value_error("weights has " + std::to_string(arr.shape(0)) + " rows, expected one per row in play (" + std::to_string(rows) + ")");
  ScoreWeights out;
  out.rows = rows;
  out.K = arr.ndim() == 1 ? 1 : (size_t)arr.shape(1);
  if (out.K < 1 || out.K > 64) value_error(std::to_string(out.K) + " weight columns: 1 to 64 are taken");
  if (rows > ((size_t)1 << 21)) value_error(std::to_string(rows) + " rows in play exceed 2^21: split the rows and add the scores");
  out.w.assign(arr.data(), arr.data() + rows * out.K);
  out.exponents.assign(out.K, 0);
  const int status = fmh_score_exponents(out.w.data(), rows, out.K, out.exponents.data());
  if (status == FMH_ERR_INVALID) value_error(fmh_last_error());  // a non-finite weight
  fmh_check(status);
  out.keep.assign(rows, 0);
  for (size_t r = 0; r < rows; ++r)
    for (size_t k = 0; k < out.K; ++k) out.keep[r] |= out.w[r * out.K + k] != 0.0 ? 1 : 0;
  return out;
}

// A result from sums that were computed before (no device).
PolygenicScore score_from_sums(const py::object& dosage_sum, const py::object& exponents, const py::object& called_sum, const py::object& called_total,
                               const string& missing, bool center, uint64_t rows_used, const py::object& n_called, const py::object& sample_dosage_sum,
                               const py::object& positions) {
  PolygenicScore out;
  out.mode = score_mode_arg(missing, center);
  out.exponents = qc_vector<int32_t>(exponents, "exponents", 0, false);
  out.K = out.exponents.size();
  if (out.K < 1 || out.K > 64) value_error(std::to_string(out.K) + " weight columns: 1 to 64 are taken");
  auto sums = [&](const py::object& obj, const char* name, size_t expect) {
    auto arr = py::array_t<long long, py::array::c_style | py::array::forcecast>::ensure(obj);
    if (!arr || (expect != (size_t)-1 && (size_t)arr.size() != expect)) value_error(string(name) + " must hold [samples][K] integers");
    return vector<long long>(arr.data(), arr.data() + arr.size());
  };
  const vector<long long> S = sums(dosage_sum, "dosage_sum", (size_t)-1);
  if (S.size() % out.K != 0) value_error("dosage_sum must hold [samples][K] integers, K = " + std::to_string(out.K));
  out.n = S.size() / out.K;
  vector<long long> C, T;
  if (out.mode != FMH_SCORE_ZERO) {
    if (called_sum.is_none()) value_error("modes mean and center need called_sum");
    C = sums(called_sum, "called_sum", S.size());
  }
  if (out.mode == FMH_SCORE_MEAN) {
    if (called_total.is_none()) value_error("mode mean needs called_total");
    T = qc_vector<long long>(called_total, "called_total", out.K, true);
  }
  out.rows_used = rows_used;
  if (!n_called.is_none()) out.n_called = qc_vector<uint64_t>(n_called, "n_called", out.n, true);
  if (!sample_dosage_sum.is_none()) out.dosage_sum = qc_vector<uint64_t>(sample_dosage_sum, "sample_dosage_sum", out.n, true);
  if (!positions.is_none()) out.positions = qc_vector<int64_t>(positions, "positions", 0, false);
  out.score.assign(out.n * out.K, 0.0);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_score_stats(S.data(), C.empty() ? nullptr : C.data(), T.empty() ? nullptr : T.data(), out.exponents.data(), out.n, out.K, out.mode,
                             out.score.data());
  }
  if (status == FMH_ERR_INVALID) value_error(fmh_last_error());
  fmh_check(status);
  return out;
}

PolygenicScore score_over_rows(const shared_ptr<DevMatrix>& dm, size_t r0, size_t rc, const vector<uint32_t>& samples, const ScoreWeights& weights, int mode,
                               vector<int64_t> positions) {
  PolygenicScore out;
  const size_t n = samples.size(), K = weights.K;
  out.n = n; out.K = K; out.mode = mode;
  out.exponents = weights.exponents;
  out.positions = std::move(positions);
  out.score.assign(n * K, 0.0);
  out.n_called.assign(n, 0);
  out.dosage_sum.assign(n, 0);
  if (!dm || rc == 0) return out;
  const bool called = mode != FMH_SCORE_ZERO;
  // the most rows whose digits and slabs one fmh_score_sums call holds under the budget (score_host.hpp's rule, the library's own)
  long long budget = 0, item_option = 0;
  fmh_check(fmh_get_option("FMH_SCORE_BUDGET_BYTES", &budget));
  fmh_check(fmh_get_option("FMH_SCORE_ITEM_ROWS", &item_option));
  const size_t item_rows = fmh_host::score_item_rows(item_option), covered = (size_t)samples.back() + 1;
  size_t chunk_rows = 1;
  for (size_t lo = 1, hi = rc; lo <= hi;) {
    const size_t mid = lo + (hi - lo) / 2;
    if (budget > 0 && fmh_host::score_call_bytes(mid, covered, K, item_rows, called) <= (size_t)budget) { chunk_rows = mid; lo = mid + 1; }
    else hi = mid - 1;
  }
  DevBuf d_sums(dm->device, 2 * n * K * sizeof(long long)), d_tracks(dm->device, 3 * chunk_rows * sizeof(uint32_t));
  DevBuf d_classes(dm->device, 3 * n * sizeof(unsigned long long));
  long long* d_s = (long long*)d_sums.p;
  long long* d_c = d_s + n * K;
  uint32_t* t = (uint32_t*)d_tracks.p;
  unsigned long long* cls = (unsigned long long*)d_classes.p;
  const fmh_genotype_site_out site{t, t + chunk_rows, t + 2 * chunk_rows};
  const fmh_genotype_sample_out sample{cls, cls + n, cls + 2 * n, nullptr};
  vector<long long> S(n * K), C(n * K), sum_s(n * K, 0), sum_c(n * K, 0), T(K), total(K, 0);
  vector<int32_t> V(chunk_rows * K), U(chunk_rows * K);
  vector<uint32_t> tracks(3 * chunk_rows);
  vector<uint8_t> used(chunk_rows);
  vector<unsigned long long> classes(3 * n);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    const int dev = dm->device;
    status = fmh_device_zero(dev, cls, 3 * n * sizeof(unsigned long long), nullptr);
    for (size_t at = 0; at < rc && status == FMH_OK; at += chunk_rows) {
      const size_t count = std::min(chunk_rows, rc - at);
      status = fmh_genotype_counts(dm->h, samples.data(), n, r0 + at, count, weights.keep.data() + at, nullptr, &site, &sample, nullptr, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, tracks.data(), t, 3 * chunk_rows * sizeof(uint32_t), nullptr);
      const uint32_t *ref = tracks.data(), *het = ref + chunk_rows, *alt = het + chunk_rows;
      if (status == FMH_OK)
        status = fmh_score_values(weights.w.data() + at * K, count, K, weights.exponents.data(), ref, het, alt, V.data(), called ? U.data() : nullptr,
                                  called ? T.data() : nullptr, used.data());
      if (status == FMH_OK)
        status = fmh_score_sums(dm->h, samples.data(), n, r0 + at, count, V.data(), called ? U.data() : nullptr, K, d_s, called ? d_c : nullptr, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, S.data(), d_s, n * K * sizeof(long long), nullptr);
      if (status == FMH_OK && called) status = fmh_copy_to_host(dev, C.data(), d_c, n * K * sizeof(long long), nullptr);
      if (status != FMH_OK) break;
      for (size_t i = 0; i < n * K; ++i) { sum_s[i] += S[i]; if (called) sum_c[i] += C[i]; }
      for (size_t k = 0; k < K && called; ++k) total[k] += T[k];
      for (size_t r = 0; r < count; ++r) out.rows_used += used[r];
    }
    if (status == FMH_OK) status = fmh_copy_to_host(dev, classes.data(), cls, 3 * n * sizeof(unsigned long long), nullptr);
    if (status == FMH_OK)
      status = fmh_score_stats(sum_s.data(), called ? sum_c.data() : nullptr, called ? total.data() : nullptr, weights.exponents.data(), n, K, mode,
                               out.score.data());
  }
  fmh_check(status);
  for (size_t i = 0; i < n; ++i) {
    out.n_called[i] = classes[i] + classes[n + i] + classes[2 * n + i];
    out.dosage_sum[i] = classes[n + i] + 2 * classes[2 * n + i];
  }
  return out;
}

PolygenicScore polygenic_score(const py::object& variants, const py::object& weights, const py::object& samples, const py::object& region,
                               const string& missing, bool center) {
  const int mode = score_mode_arg(missing, center);
  auto store = store_from_python(variants);
  if (store->S != 0 && store->P != 2) value_error("the polygenic score takes diploid genotypes (ploidy 2), got ploidy " + std::to_string(store->P));
  const vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  shared_ptr<const Store> sub = store;
  bool empty = store->S == 0;
  if (!empty && !region.is_none()) {
    const Region reg = build_region(region);
    const vector<int64_t> rows = region_len(reg) > 0 ? region_rows(*store, reg.start, reg.end) : vector<int64_t>();
    if (rows.empty()) empty = true;
    else sub = store_subset(store, rows);
  }
  const ScoreWeights w = score_weights_arg(weights, empty ? 0 : (size_t)sub->S);
  if (list.empty()) value_error("at least one sample is required for a polygenic score");
  if (empty) return score_over_rows(nullptr, 0, 0, list, w, mode, {});
  auto [dm, r0, rc] = sub->device_rows();
  vector<int64_t> positions(sub->positions.begin(), sub->positions.begin() + (std::ptrdiff_t)std::min<size_t>(rc, sub->positions.size()));
  return score_over_rows(dm, r0, rc, list, w, mode, std::move(positions));
}

// the samples BOTH of whose haplotypes belong to the population, ascending, over its resident matrix: Population.genotype_qc's rule
PolygenicScore population_polygenic_score(const Population& pop, const py::object& weights, const string& missing, bool center) {
  const int mode = score_mode_arg(missing, center);
  const int64_t ploidy = pop.dense ? pop.dense->ploidy : pop.store->P;
  const size_t count = pop.dense ? (size_t)pop.dense->variants : (size_t)pop.store->S;
  if (count != 0 && ploidy != 2) value_error("the polygenic score takes diploid genotypes (ploidy 2), got ploidy " + std::to_string(ploidy));
  const int64_t limit = pop.dense ? pop.dense->samples : pop.store->first_sample_count();
  vector<uint8_t> sides((size_t)std::max<int64_t>(limit, 0), 0);
  for (auto& h : pop.haplotypes)
    if (h.first >= 0 && h.first < limit) sides[(size_t)h.first] |= h.second == kLeft ? 1 : 2;
  vector<uint32_t> list;
  for (size_t s = 0; s < sides.size(); ++s)
    if (sides[s] == 3) list.push_back((uint32_t)s);
  const ScoreWeights w = score_weights_arg(weights, count);
  if (list.empty()) value_error("at least one sample with both haplotypes in the population is required for a polygenic score");
  if (count == 0) return score_over_rows(nullptr, 0, 0, list, w, mode, {});
  const ResidentRows rows = resident_rows_of(pop);
  const vector<int64_t>& all = pop.store->positions;
  vector<int64_t> positions(all.begin(), all.begin() + (std::ptrdiff_t)std::min(rows.rc, all.size()));
  return score_over_rows(rows.dm, rows.r0, rows.rc, list, w, mode, std::move(positions));
}

void bind_score(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<PolygenicScore>(m, "PolygenicScore")
      .def_static("from_sums", &score_from_sums, py::arg("dosage_sum"), py::arg("exponents"), py::arg("called_sum") = py::none(),
                  py::arg("called_total") = py::none(), py::arg("missing") = "mean", py::arg("center") = false, py::arg("rows_used") = 0,
                  py::arg("n_called") = py::none(), py::arg("sample_dosage_sum") = py::none(), py::arg("positions") = py::none())
      .def_property_readonly("score", [](const PolygenicScore& a) { return a.table(false); })
      .def_property_readonly("average", [](const PolygenicScore& a) { return a.table(true); })
      .def_property_readonly("n_called", [](const PolygenicScore& a) { return qc_array(a.n_called); })
      .def_property_readonly("dosage_sum", [](const PolygenicScore& a) { return qc_array(a.dosage_sum); })
      .def_property_readonly("rows_used", [](const PolygenicScore& a) { return a.rows_used; })
      .def_property_readonly("exponents", [](const PolygenicScore& a) { return qc_array(a.exponents); })
      .def_property_readonly("positions", [](const PolygenicScore& a) { return qc_array(a.positions); })
      .def_property_readonly("mode", [](const PolygenicScore& a) { return string(a.mode_name()); })
      .def("__len__", [](const PolygenicScore& a) { return a.n; })
      .def("__repr__", &PolygenicScore::repr);
  m.def("polygenic_score", &polygenic_score, py::arg("variants"), py::arg("weights"), py::arg("samples") = py::none(), py::arg("region") = py::none(),
        py::arg("missing") = "mean", py::arg("center") = false);
  population.def("polygenic_score", &population_polygenic_score, py::arg("weights"), py::arg("missing") = "mean", py::arg("center") = false);
}
