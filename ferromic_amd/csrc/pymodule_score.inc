// pymodule_score.inc — ferromic.polygenic_score, Population.polygenic_score and the PolygenicScore result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample rules and chunk tracks it uses).  An addition to the reference's
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
  fmh_check_args(status);  // a non-finite weight
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
  out.exponents = vector_arg<int32_t>(exponents, "exponents", 0, false);
  out.K = out.exponents.size();
  if (out.K < 1 || out.K > 64) value_error(std::to_string(out.K) + " weight columns: 1 to 64 are taken");
  const vector<long long> S = i64_table_arg(dosage_sum, "dosage_sum", kAnySize, "hold [samples][K] integers");
  if (S.size() % out.K != 0) value_error("dosage_sum must hold [samples][K] integers, K = " + std::to_string(out.K));
  out.n = S.size() / out.K;
  vector<long long> C, T;
  if (out.mode != FMH_SCORE_ZERO) {
    if (called_sum.is_none()) value_error("modes mean and center need called_sum");
    C = i64_table_arg(called_sum, "called_sum", S.size(), "hold [samples][K] integers");
  }
  if (out.mode == FMH_SCORE_MEAN) {
    if (called_total.is_none()) value_error("mode mean needs called_total");
    T = vector_arg<long long>(called_total, "called_total", out.K, true);
  }
  out.rows_used = rows_used;
  if (!n_called.is_none()) out.n_called = vector_arg<uint64_t>(n_called, "n_called", out.n, true);
  if (!sample_dosage_sum.is_none()) out.dosage_sum = vector_arg<uint64_t>(sample_dosage_sum, "sample_dosage_sum", out.n, true);
  if (!positions.is_none()) out.positions = vector_arg<int64_t>(positions, "positions", 0, false);
  out.score.assign(out.n * out.K, 0.0);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_score_stats(S.data(), C.empty() ? nullptr : C.data(), T.empty() ? nullptr : T.data(), out.exponents.data(), out.n, out.K, out.mode,
                             out.score.data());
  }
  fmh_check_args(status);
  return out;
}

PolygenicScore score_over_rows(const RowsInPlay& in_play, const vector<uint32_t>& samples, const ScoreWeights& weights, int mode) {
  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  PolygenicScore out;
  const size_t n = samples.size(), K = weights.K;
  out.n = n; out.K = K; out.mode = mode;
  out.exponents = weights.exponents;
  out.positions = in_play.positions_copy();
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
  DevBuf d_sums(dm->device, 2 * n * K * sizeof(long long));
  ChunkTracks tracks(dm->device, chunk_rows);
  DevBuf d_classes(dm->device, 3 * n * sizeof(unsigned long long));
  long long* d_s = (long long*)d_sums.p;
  long long* d_c = d_s + n * K;
  unsigned long long* cls = (unsigned long long*)d_classes.p;
  const fmh_genotype_sample_out sample{cls, cls + n, cls + 2 * n, nullptr};
  vector<long long> S(n * K), C(n * K), sum_s(n * K, 0), sum_c(n * K, 0), T(K), total(K, 0);
  vector<int32_t> V(chunk_rows * K), U(chunk_rows * K);
  vector<uint8_t> used(chunk_rows);
  vector<unsigned long long> classes(3 * n);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    const int dev = dm->device;
    status = fmh_device_zero(dev, cls, 3 * n * sizeof(unsigned long long), nullptr);
    for (size_t at = 0; at < rc && status == FMH_OK; at += chunk_rows) {
      const size_t count = std::min(chunk_rows, rc - at);
      status = fmh_genotype_counts(dm->h, samples.data(), n, r0 + at, count, weights.keep.data() + at, nullptr, &tracks.site, &sample, nullptr, nullptr);
      if (status == FMH_OK) status = tracks.download();
      if (status == FMH_OK)
        status = fmh_score_values(weights.w.data() + at * K, count, K, weights.exponents.data(), tracks.ref(), tracks.het(), tracks.alt(), V.data(), called ? U.data() : nullptr,
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
  diploid_only(store->P, (size_t)store->S, "the polygenic score takes");
  const vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  const RowsInPlay rows = rows_in_play(store, region);
  const ScoreWeights w = score_weights_arg(weights, rows.count);
  if (list.empty()) value_error("at least one sample is required for a polygenic score");
  return score_over_rows(rows, list, w, mode);
}

PolygenicScore population_polygenic_score(const Population& pop, const py::object& weights, const string& missing, bool center) {
  const int mode = score_mode_arg(missing, center);
  diploid_only(pop, "the polygenic score takes");
  const vector<uint32_t> list = population_samples(pop);
  const RowsInPlay rows = rows_in_play(pop);
  const ScoreWeights w = score_weights_arg(weights, rows.count);
  if (list.empty()) value_error("at least one sample with both haplotypes in the population is required for a polygenic score");
  return score_over_rows(rows, list, w, mode);
}

void bind_score(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<PolygenicScore>(m, "PolygenicScore")
      .def_static("from_sums", &score_from_sums, py::arg("dosage_sum"), py::arg("exponents"), py::arg("called_sum") = py::none(),
                  py::arg("called_total") = py::none(), py::arg("missing") = "mean", py::arg("center") = false, py::arg("rows_used") = 0,
                  py::arg("n_called") = py::none(), py::arg("sample_dosage_sum") = py::none(), py::arg("positions") = py::none())
      .def_property_readonly("score", [](const PolygenicScore& a) { return a.table(false); })
      .def_property_readonly("average", [](const PolygenicScore& a) { return a.table(true); })
      .def_property_readonly("n_called", [](const PolygenicScore& a) { return array_of(a.n_called); })
      .def_property_readonly("dosage_sum", [](const PolygenicScore& a) { return array_of(a.dosage_sum); })
      .def_property_readonly("rows_used", [](const PolygenicScore& a) { return a.rows_used; })
      .def_property_readonly("exponents", [](const PolygenicScore& a) { return array_of(a.exponents); })
      .def_property_readonly("positions", [](const PolygenicScore& a) { return array_of(a.positions); })
      .def_property_readonly("mode", [](const PolygenicScore& a) { return string(a.mode_name()); })
      .def("__len__", [](const PolygenicScore& a) { return a.n; })
      .def("__repr__", &PolygenicScore::repr);
  m.def("polygenic_score", &polygenic_score, py::arg("variants"), py::arg("weights"), py::arg("samples") = py::none(), py::arg("region") = py::none(),
        py::arg("missing") = "mean", py::arg("center") = false);
  population.def("polygenic_score", &population_polygenic_score, py::arg("weights"), py::arg("missing") = "mean", py::arg("center") = false);
}
