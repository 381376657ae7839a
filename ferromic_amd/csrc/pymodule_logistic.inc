// pymodule_logistic.inc — ferromic.logistic_scan, Population.logistic_scan and the LogisticScan result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample rules and chunk tracks it uses).  An addition to the
// reference's surface; the definition is include/ferromic_hip.h's (fmh_logistic_null, fmh_assoc_homalt_sums, fmh_logistic_score,
// fmh_logistic_stats).  The null models are fitted on the host once; the exact sums AND their reduction to a score and a variance per (row,
// phenotype) run on the device, row chunk by row chunk and phenotype batch by phenotype batch: only two doubles per (row, phenotype) and the
// three tracks of a chunk come down.  The GIL is released around the C calls.

struct LogisticScan {
  size_t rows = 0, n_phenotypes = 0;
  uint64_t n_samples = 0;
  vector<double> score, variance, chi2, z, p, beta, se;  // [rows][P]
  vector<uint32_t> n_called;                             // [rows]
  vector<double> alt_frequency;                          // [rows]
  vector<int64_t> positions;                             // [rows] (empty when built from sums without them)
  vector<uint64_t> n_cases;                              // [P]
  vector<uint8_t> fitted;                                // [P]
  vector<int32_t> iterations, reason;                    // [P]
  vector<int64_t> kept, dropped;                         // covariate column numbers

  void reserve_rows(size_t r, size_t P) {
    rows = r; n_phenotypes = P;
    for (vector<double>* v : {&score, &variance, &chi2, &z, &p, &beta, &se}) v->assign(r * P, 0.0);
    n_called.assign(r, 0);
    alt_frequency.assign(r, 0.0);
  }
  py::array_t<double> table(const vector<double>& v) const {
    py::array_t<double> out({(py::ssize_t)rows, (py::ssize_t)n_phenotypes});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(double));
    return out;
  }
  py::array_t<bool> fitted_array() const {
    py::array_t<bool> out((py::ssize_t)fitted.size());
    for (size_t i = 0; i < fitted.size(); ++i) out.mutable_data()[i] = fitted[i] != 0;
    return out;
  }
  // the statistics of every entry, then NaN columns for the phenotypes that were not fitted; a library status
  int finish() {
    const int status = fmh_logistic_stats(score.data(), variance.data(), score.size(), chi2.data(), z.data(), p.data(), beta.data(), se.data());
    if (status != FMH_OK) return status;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t ph = 0; ph < n_phenotypes; ++ph)
      if (!fitted[ph])
        for (vector<double>* v : {&score, &variance, &chi2, &z, &p, &beta, &se})
          for (size_t r = 0; r < rows; ++r) (*v)[r * n_phenotypes + ph] = nan;
    return FMH_OK;
  }
  string repr() const {
    size_t n_fitted = 0;
    for (uint8_t f : fitted) n_fitted += f ? 1 : 0;
    return "LogisticScan(samples=" + std::to_string(n_samples) + ", sites=" + std::to_string(rows) + ", phenotypes=" + std::to_string(n_phenotypes) +
           ", fitted=" + std::to_string(n_fitted) + ", covariates=" + std::to_string(kept.size()) + ")";
  }
};

// what fmh_logistic_null made of the phenotypes and covariates
struct LogisticModel {
  size_t n = 0, c = 0, P = 0;
  vector<int32_t> values, exponent;  // values: batches of [n][Pb * (c + 3)]; exponent, total: [P][c + 3]
  vector<long long> total;
  vector<uint8_t> fitted;
  vector<int32_t> reason, iterations;
  vector<uint64_t> n_cases;
  vector<int64_t> kept, dropped;
  size_t width() const { return c + 3; }
  size_t batch() const { return 64 / width(); }
};

// [n] or [n][P] / [n][c_in] f64, in the order of the selected samples; every argument error before any device use
LogisticModel logistic_model(const py::object& phenotypes, const py::object& covariates, size_t n) {
  auto y = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(phenotypes);
  if (!y || (y.ndim() != 1 && y.ndim() != 2)) value_error("phenotypes must be a numeric array [n] or [n][P]");
  if ((size_t)y.shape(0) != n) value_error("phenotypes has " + std::to_string(y.shape(0)) + " rows, expected one per selected sample (" + std::to_string(n) + ")");
  LogisticModel out;
  out.n = n;
  out.P = y.ndim() == 1 ? 1 : (size_t)y.shape(1);
  if (out.P == 0) value_error("at least one phenotype is required");
  size_t cin = 0;
  py::array_t<double, py::array::c_style | py::array::forcecast> x;
  if (!covariates.is_none()) {
    x = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(covariates);
    if (!x || x.ndim() != 2) value_error("covariates must be a numeric array [n][c_in]");
    if ((size_t)x.shape(0) != n) value_error("covariates has " + std::to_string(x.shape(0)) + " rows, expected one per selected sample (" + std::to_string(n) + ")");
    cin = (size_t)x.shape(1);
  }
  if (n == 0) value_error("at least one sample is required for a logistic scan");
  out.values.assign(n * out.P * (cin + 3), 0);
  out.exponent.assign(out.P * (cin + 3), 0);
  out.total.assign(out.P * (cin + 3), 0);
  out.fitted.assign(out.P, 0);
  out.reason.assign(out.P, 0);
  out.iterations.assign(out.P, 0);
  out.n_cases.assign(out.P, 0);
  vector<uint8_t> dropped(cin, 0);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_logistic_null(y.data(), cin ? x.data() : nullptr, n, out.P, cin, out.values.data(), out.exponent.data(), out.total.data(), out.fitted.data(),
                               out.reason.data(), out.iterations.data(), (uint64_t*)out.n_cases.data(), &out.c, cin ? dropped.data() : nullptr);
  }
  fmh_check_args(status);  // a phenotype that is not 0 / 1, a non-finite covariate, too few samples: the caller's
  for (size_t j = 0; j < cin; ++j) (dropped[j] ? out.dropped : out.kept).push_back((int64_t)j);
  return out;
}

void logistic_take_model(LogisticScan& out, const LogisticModel& model) {
  out.n_samples = model.n;
  out.kept = model.kept;
  out.dropped = model.dropped;
  out.fitted = model.fitted;
  out.reason = model.reason;
  out.iterations = model.iterations;
  out.n_cases = model.n_cases;
}

// N and the alt allele frequency of rows [at, at + count) from the tracks; a library status (callable with the GIL released)
int logistic_site_columns(LogisticScan& out, size_t at, size_t count, const uint32_t* ref, const uint32_t* het, const uint32_t* alt) {
  for (size_t i = 0; i < count; ++i) out.n_called[at + i] = ref[i] + het[i] + alt[i];
  const fmh_genotype_site_stats_out site{nullptr, out.alt_frequency.data() + at, nullptr, nullptr, nullptr};
  return fmh_genotype_site_stats(ref, het, alt, count, out.n_samples, &site);
}

// A result from sums that were computed before (no device): the host twin of the device reduction.  dosage_sum and called_sum hold
// [rows][P][c + 3] integers (phenotype after phenotype, as the batches of fmh_logistic_null laid side by side), homalt_sum [rows][P], total
// and exponent [P][c + 3].
LogisticScan logistic_from_sums(const py::object& dosage_sum, const py::object& called_sum, const py::object& homalt_sum, const py::object& hom_ref,
                                const py::object& het, const py::object& hom_alt, const py::object& total, const py::object& exponent, uint64_t n_samples,
                                size_t n_basis, const py::object& fitted, const py::object& n_cases, const py::object& iterations, const py::object& positions,
                                const py::object& covariates_kept, const py::object& covariates_dropped) {
  LogisticScan out;
  const vector<uint32_t> ref = vector_arg<uint32_t>(hom_ref, "hom_ref", 0, false);
  const vector<uint32_t> h = vector_arg<uint32_t>(het, "het", ref.size(), true), alt = vector_arg<uint32_t>(hom_alt, "hom_alt", ref.size(), true);
  if (n_basis + 3 > 64) value_error("n_basis + 3 exceeds 64 value columns");
  const size_t rows = ref.size(), W = n_basis + 3, B = 64 / W;
  auto flat = [](const py::object& obj, const char* name) { return i64_table_arg(obj, name, kAnySize, "be an integer array"); };
  const vector<long long> tot = flat(total, "total");
  if (tot.empty() || tot.size() % W != 0) value_error("total must hold [P][c + 3] integers with P >= 1");
  const size_t P = tot.size() / W;
  auto ev = py::array_t<int32_t, py::array::c_style | py::array::forcecast>::ensure(exponent);
  if (!ev || (size_t)ev.size() != P * W) value_error("exponent must hold [P][c + 3] = " + std::to_string(P * W) + " integers");
  const vector<long long> S = flat(dosage_sum, "dosage_sum"), C = flat(called_sum, "called_sum"), H = flat(homalt_sum, "homalt_sum");
  if (S.size() != rows * P * W || C.size() != rows * P * W) value_error("dosage_sum and called_sum must hold [rows][P][c + 3] = " + std::to_string(rows * P * W) + " integers");
  if (H.size() != rows * P) value_error("homalt_sum must hold [rows][P] = " + std::to_string(rows * P) + " integers");
  out.fitted.assign(P, 1);
  if (!fitted.is_none()) {
    const vector<uint8_t> f = vector_arg<uint8_t>(fitted, "fitted", P, true);
    for (size_t i = 0; i < P; ++i) out.fitted[i] = f[i] ? 1 : 0;
  }
  out.n_cases = n_cases.is_none() ? vector<uint64_t>(P, 0) : vector_arg<uint64_t>(n_cases, "n_cases", P, true);
  out.iterations = iterations.is_none() ? vector<int32_t>(P, 0) : vector_arg<int32_t>(iterations, "iterations", P, true);
  out.reason.assign(P, 0);
  if (!positions.is_none()) out.positions = vector_arg<int64_t>(positions, "positions", rows, true);
  if (!covariates_kept.is_none()) out.kept = vector_arg<int64_t>(covariates_kept, "covariates_kept", n_basis, true);
  if (!covariates_dropped.is_none()) out.dropped = vector_arg<int64_t>(covariates_dropped, "covariates_dropped", 0, false);
  out.n_samples = n_samples;
  out.reserve_rows(rows, P);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    vector<long long> s, c, hb;
    vector<double> u, v;
    for (size_t first = 0; first < P && status == FMH_OK; first += B) {
      const size_t Pb = std::min(B, P - first), K = Pb * W;
      s.resize(rows * K); c.resize(rows * K); hb.resize(rows * Pb); u.resize(rows * Pb); v.resize(rows * Pb);
      for (size_t r = 0; r < rows; ++r) {
        memcpy(s.data() + r * K, S.data() + (r * P + first) * W, K * sizeof(long long));
        memcpy(c.data() + r * K, C.data() + (r * P + first) * W, K * sizeof(long long));
        memcpy(hb.data() + r * Pb, H.data() + r * P + first, Pb * sizeof(long long));
      }
      status = fmh_logistic_score_host(s.data(), c.data(), hb.data(), ref.data(), h.data(), alt.data(), rows, tot.data() + first * W, ev.data() + first * W,
                                       n_basis, Pb, u.data(), v.data());
      for (size_t r = 0; r < rows && status == FMH_OK; ++r)
        for (size_t q = 0; q < Pb; ++q) {
          out.score[r * P + first + q] = u[r * Pb + q];
          out.variance[r * P + first + q] = v[r * Pb + q];
        }
    }
    if (status == FMH_OK) status = out.finish();
    if (status == FMH_OK) status = logistic_site_columns(out, 0, rows, ref.data(), h.data(), alt.data());
  }
  fmh_check_args(status);
  return out;
}

LogisticScan logistic_over_rows(const RowsInPlay& in_play, const vector<uint32_t>& samples, const LogisticModel& model) {
  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  LogisticScan out;
  const size_t n = model.n, c = model.c, P = model.P, W = model.width(), B = model.batch(), Bmax = std::min(B, P), Kmax = Bmax * W;
  logistic_take_model(out, model);
  out.positions = in_play.positions_copy();
  out.reserve_rows(dm ? rc : 0, P);
  if (!dm || rc == 0) return out;
  // per row of a chunk: S and C [Kmax], H [Bmax], score and variance [Bmax]
  const size_t row_bytes = (2 * Kmax + 3 * Bmax) * sizeof(long long);
  const size_t chunk_rows = chunk_rows_under("FMH_ASSOC_BUDGET_BYTES", rc, row_bytes);
  DevBuf d_sums(dm->device, chunk_rows * row_bytes);
  long long* d_s = (long long*)d_sums.p;
  long long* d_c = d_s + chunk_rows * Kmax;
  long long* d_h = d_c + chunk_rows * Kmax;
  double* d_u = (double*)(d_h + chunk_rows * Bmax);
  double* d_v = d_u + chunk_rows * Bmax;
  ChunkTracks tracks(dm->device, chunk_rows);
  const fmh_genotype_site_out& site = tracks.site;
  vector<double> U(chunk_rows * Bmax), V(chunk_rows * Bmax);
  vector<int32_t> wcol(n * Bmax);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    const int dev = dm->device;
    for (size_t at = 0; at < rc && status == FMH_OK; at += chunk_rows) {
      const size_t count = std::min(chunk_rows, rc - at);
      status = fmh_genotype_counts(dm->h, samples.data(), n, r0 + at, count, nullptr, nullptr, &site, nullptr, nullptr, nullptr);
      for (size_t first = 0; first < P && status == FMH_OK; first += B) {
        const size_t Pb = std::min(B, P - first), K = Pb * W;
        const int32_t* values = model.values.data() + n * W * first;
        for (size_t i = 0; i < n; ++i)
          for (size_t q = 0; q < Pb; ++q) wcol[i * Pb + q] = values[i * K + q * W + c + 2];  // the batch's w columns
        status = fmh_assoc_sums(dm->h, samples.data(), n, r0 + at, count, values, K, d_s, d_c, nullptr);
        if (status == FMH_OK) status = fmh_assoc_homalt_sums(dm->h, samples.data(), n, r0 + at, count, wcol.data(), Pb, d_h, nullptr);
        if (status == FMH_OK)
          status = fmh_logistic_score(d_s, d_c, d_h, site.d_hom_ref, site.d_het, site.d_hom_alt, count, model.total.data() + first * W,
                                      model.exponent.data() + first * W, c, Pb, d_u, d_v, dev, nullptr);
        if (status == FMH_OK) status = fmh_copy_to_host(dev, U.data(), d_u, count * Pb * sizeof(double), nullptr);
        if (status == FMH_OK) status = fmh_copy_to_host(dev, V.data(), d_v, count * Pb * sizeof(double), nullptr);
        for (size_t i = 0; i < count && status == FMH_OK; ++i)
          for (size_t q = 0; q < Pb; ++q) {
            out.score[(at + i) * P + first + q] = U[i * Pb + q];
            out.variance[(at + i) * P + first + q] = V[i * Pb + q];
          }
      }
      if (status == FMH_OK) status = tracks.download();
      if (status == FMH_OK) status = logistic_site_columns(out, at, count, tracks.ref(), tracks.het(), tracks.alt());
    }
    if (status == FMH_OK) status = out.finish();
  }
  fmh_check(status);
  return out;
}

LogisticScan logistic_scan(const py::object& variants, const py::object& phenotypes, const py::object& covariates, const py::object& samples,
                           const py::object& region) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "the logistic scan takes");
  const vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  const LogisticModel model = logistic_model(phenotypes, covariates, list.size());
  return logistic_over_rows(rows_in_play(store, region), list, model);
}

LogisticScan population_logistic_scan(const Population& pop, const py::object& phenotypes, const py::object& covariates) {
  diploid_only(pop, "the logistic scan takes");
  const vector<uint32_t> list = population_samples(pop);
  const LogisticModel model = logistic_model(phenotypes, covariates, list.size());
  return logistic_over_rows(rows_in_play(pop), list, model);
}

void bind_logistic(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<LogisticScan>(m, "LogisticScan")
      .def_static("from_sums", &logistic_from_sums, py::arg("dosage_sum"), py::arg("called_sum"), py::arg("homalt_sum"), py::arg("hom_ref"), py::arg("het"),
                  py::arg("hom_alt"), py::arg("total"), py::arg("exponent"), py::arg("n_samples"), py::arg("n_basis"), py::arg("fitted") = py::none(),
                  py::arg("n_cases") = py::none(), py::arg("iterations") = py::none(), py::arg("positions") = py::none(),
                  py::arg("covariates_kept") = py::none(), py::arg("covariates_dropped") = py::none())
      .def_property_readonly("score", [](const LogisticScan& a) { return a.table(a.score); })
      .def_property_readonly("variance", [](const LogisticScan& a) { return a.table(a.variance); })
      .def_property_readonly("chi2", [](const LogisticScan& a) { return a.table(a.chi2); })
      .def_property_readonly("z", [](const LogisticScan& a) { return a.table(a.z); })
      .def_property_readonly("p", [](const LogisticScan& a) { return a.table(a.p); })
      .def_property_readonly("beta", [](const LogisticScan& a) { return a.table(a.beta); })
      .def_property_readonly("se", [](const LogisticScan& a) { return a.table(a.se); })
      .def_property_readonly("n_called", [](const LogisticScan& a) { return array_of(a.n_called); })
      .def_property_readonly("alt_frequency", [](const LogisticScan& a) { return array_of(a.alt_frequency); })
      .def_property_readonly("positions", [](const LogisticScan& a) { return array_of(a.positions); })
      .def_property_readonly("n_cases", [](const LogisticScan& a) { return array_of(a.n_cases); })
      .def_property_readonly("fitted", [](const LogisticScan& a) { return a.fitted_array(); })
      .def_property_readonly("iterations", [](const LogisticScan& a) { return array_of(a.iterations); })
      .def_property_readonly("reason", [](const LogisticScan& a) { return array_of(a.reason); })
      .def_property_readonly("covariates_kept", [](const LogisticScan& a) { return array_of(a.kept); })
      .def_property_readonly("covariates_dropped", [](const LogisticScan& a) { return array_of(a.dropped); })
      .def("__len__", [](const LogisticScan& a) { return a.rows; })
      .def("__repr__", &LogisticScan::repr);
  m.def("logistic_scan", &logistic_scan, py::arg("variants"), py::arg("phenotypes"), py::arg("covariates") = py::none(), py::arg("samples") = py::none(),
        py::arg("region") = py::none());
  population.def("logistic_scan", &population_logistic_scan, py::arg("phenotypes"), py::arg("covariates") = py::none());
}
