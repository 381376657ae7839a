// pymodule_ldscore.inc — ferromic.ld_scores, Population.ld_scores, ferromic.ld_score_regression and the LdScores / LdScoreRegression results
// (included inside pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample and sites rules it uses, and
// pymodule_segments.inc for the positions in play).  An addition to the reference's surface: it has no LD scores; the definition is
// include/ferromic_hip.h's (fmh_ld_scores, fmh_ld_score_values, fmh_ldsc_regress).  Every sum, score and estimate comes from the library; the
// GIL is released around the C calls.  Positions go to the library relative to the first row in play.  A request without a kept row is
// answered without a device.

struct LdScoreRegression {
  fmh_ldsc_out out{};
  py::object fixed = py::none();
  string repr() const {
    char text[200];
    snprintf(text, sizeof text, "LdScoreRegression(h2=%.6g, h2_se=%.6g, intercept=%.6g, intercept_se=%.6g, n_used=%llu, blocks=%llu)", out.h2, out.h2_se, out.intercept,
             out.intercept_se, (unsigned long long)out.n_used, (unsigned long long)out.blocks);
    return text;
  }
};

vector<double> f64_sites_arg(const py::object& obj, const char* name, size_t expect) {
  auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(obj);
  if (!arr || arr.ndim() != 1) value_error(string(name) + " must be a one-dimensional float array");
  if ((size_t)arr.shape(0) != expect) value_error(string(name) + " has " + std::to_string(arr.shape(0)) + " entries for " + std::to_string(expect) + " sites");
  return vector<double>(arr.data(), arr.data() + expect);
}

double f64_number_arg(const py::object& obj, const char* name) {
  try {
    return obj.cast<double>();
  } catch (const py::cast_error&) {
    value_error(string(name) + " must be a number");
  }
  return 0.0;
}

// the regression's arguments, checked here so that every refusal is a ValueError with the library's words
LdScoreRegression ld_score_regress(const vector<double>& chi2, const vector<double>& scores, const py::object& n_samples, const py::object& m_sites, int64_t blocks,
                                   const py::object& intercept, const py::object& weights) {
  LdScoreRegression r;
  const size_t K = scores.size();
  vector<double> w;
  if (!weights.is_none()) w = f64_sites_arg(weights, "weights", K);
  if (n_samples.is_none()) value_error("n_samples is required");
  const double N = f64_number_arg(n_samples, "n_samples");
  double M = 0.0;
  if (m_sites.is_none()) {
    for (double v : scores) M += std::isfinite(v);
  } else {
    M = f64_number_arg(m_sites, "m_sites");
  }
  if (blocks < 0) value_error("blocks must not be negative");
  double fixed = 0.0;
  if (!intercept.is_none()) fixed = f64_number_arg(intercept, "intercept");
  r.fixed = intercept;
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_ldsc_regress(chi2.data(), scores.data(), weights.is_none() ? nullptr : w.data(), K, N, M, (uint64_t)blocks, intercept.is_none() ? nullptr : &fixed, &r.out);
  }
  fmh_check_args(status);
  return r;
}

struct LdScores {
  vector<int64_t> q;
  vector<uint32_t> partners, counted;
  vector<double> scores;
  vector<int64_t> positions;
  int64_t window = 0;
  bool adjusted = true;
  size_t n_samples = 0;

  size_t m_sites() const {
    size_t m = 0;
    for (double v : scores) m += std::isfinite(v);
    return m;
  }
  void fill_scores() {
    scores.assign(q.size(), 0.0);
    fmh_check_args(fmh_ld_score_values(q.data(), counted.data(), q.size(), scores.data()));
  }
  string repr() const {
    return "LdScores(rows=" + std::to_string(q.size()) + ", scored=" + std::to_string(m_sites()) + ", window=" + std::to_string(window) +
           ", adjusted=" + (adjusted ? "True" : "False") + ", n_samples=" + std::to_string(n_samples) + ")";
  }
};

int64_t ldscore_window_arg(int64_t window) {
  if (window < 0 || window > (int64_t)0xFFFFFFFFll) value_error("window must be within 0 .. 2^32 - 1");
  return window;
}

LdScores ld_scores_over_rows(const RowsInPlay& in_play, vector<uint32_t> samples, const py::object& sites, int64_t window, bool adjust, const char* no_sample) {
  LdScores out;
  const size_t n = samples.size();
  if (n == 0) value_error(no_sample);
  const size_t rc = in_play.count;
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  out.window = window;
  out.adjusted = adjust;
  out.n_samples = n;
  out.positions = in_play.positions_copy();
  out.q.assign(rc, 0);
  out.partners.assign(rc, 0);
  out.counted.assign(rc, 0);
  out.scores.assign(rc, std::numeric_limits<double>::quiet_NaN());
  if (rc == 0) return out;
  check_positions_in_play(out.positions, "the LD scores need", "score");
  size_t kept = 0;
  for (size_t r = 0; r < rc; ++r) kept += !masked || keep[r];
  if (kept == 0) return out;  // nothing for a device to do

  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  if (!dm || rows.rc < rc) throw std::runtime_error("the resident matrix holds fewer rows than are in play");
  const vector<uint32_t> device_x = device_positions(out.positions, dm->variants, rows.r0);
  fmh_ldscore_params P{};
  P.window = (uint32_t)window;
  P.flags = adjust ? FMH_LDSCORE_ADJUST : 0u;
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_ld_scores(dm->h, samples.data(), n, rows.r0, rc, masked ? keep.data() : nullptr, device_x.data(), &P, out.q.data(), out.partners.data(), out.counted.data(),
                           nullptr);
  }
  fmh_check_args(status);
  out.fill_scores();
  return out;
}

void bind_ldscore(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<LdScoreRegression>(m, "LdScoreRegression")
      .def_property_readonly("h2", [](const LdScoreRegression& r) { return r.out.h2; })
      .def_property_readonly("h2_se", [](const LdScoreRegression& r) { return r.out.h2_se; })
      .def_property_readonly("intercept", [](const LdScoreRegression& r) { return r.out.intercept; })
      .def_property_readonly("intercept_se", [](const LdScoreRegression& r) { return r.out.intercept_se; })
      .def_property_readonly("ratio", [](const LdScoreRegression& r) { return r.out.ratio; })
      .def_property_readonly("mean_chi2", [](const LdScoreRegression& r) { return r.out.mean_chi2; })
      .def_property_readonly("lambda_gc", [](const LdScoreRegression& r) { return r.out.lambda_gc; })
      .def_property_readonly("n_used", [](const LdScoreRegression& r) { return r.out.n_used; })
      .def_property_readonly("blocks", [](const LdScoreRegression& r) { return r.out.blocks; })
      .def_property_readonly("fixed_intercept", [](const LdScoreRegression& r) { return r.fixed; })
      .def("__repr__", &LdScoreRegression::repr);

  py::class_<LdScores>(m, "LdScores")
      .def_static("from_q",
                  [](const py::object& q, const py::object& counted, const py::object& partners, const py::object& positions, int64_t window, bool adjusted,
                     int64_t n_samples) {
                    LdScores out;
                    out.q = vector_arg<int64_t>(q, "q", 0, false);
                    const size_t K = out.q.size();
                    out.counted = vector_arg<uint32_t>(counted, "counted", K, true);
                    if (partners.is_none()) out.partners = out.counted;
                    else out.partners = vector_arg<uint32_t>(partners, "partners", K, true);
                    for (size_t k = 0; k < K; ++k)
                      if (out.counted[k] > out.partners[k]) value_error("counted exceeds partners at row " + std::to_string(k));
                    if (positions.is_none()) for (size_t k = 0; k < K; ++k) out.positions.push_back((int64_t)k);
                    else out.positions = vector_arg<int64_t>(positions, "positions", K, true);
                    out.window = ldscore_window_arg(window);
                    if (n_samples < 0) value_error("n_samples must not be negative");
                    out.adjusted = adjusted;
                    out.n_samples = (size_t)n_samples;
                    out.fill_scores();
                    return out;
                  },
                  py::arg("q"), py::arg("counted"), py::arg("partners") = py::none(), py::arg("positions") = py::none(), py::arg("window") = 1000000,
                  py::arg("adjusted") = true, py::arg("n_samples") = 0)
      .def_property_readonly("scores", [](const LdScores& r) { return array_of(r.scores); })
      .def_property_readonly("q", [](const LdScores& r) { return array_of(r.q); })
      .def_property_readonly("partners", [](const LdScores& r) { return array_of(r.partners); })
      .def_property_readonly("counted", [](const LdScores& r) { return array_of(r.counted); })
      .def_property_readonly("positions", [](const LdScores& r) { return array_of(r.positions); })
      .def_readonly("window", &LdScores::window)
      .def_readonly("adjusted", &LdScores::adjusted)
      .def_readonly("n_samples", &LdScores::n_samples)
      .def_property_readonly("m_sites", &LdScores::m_sites)
      .def("regression",
           [](const LdScores& r, const py::object& chi2, const py::object& n_samples, const py::object& m_sites, int64_t blocks, const py::object& intercept,
              const py::object& weights) {
             const vector<double> y = f64_sites_arg(chi2, "chi2", r.q.size());
             return ld_score_regress(y, r.scores, n_samples.is_none() ? py::object(py::int_(r.n_samples)) : n_samples, m_sites, blocks, intercept, weights);
           },
           py::arg("chi2"), py::arg("n_samples") = py::none(), py::arg("m_sites") = py::none(), py::arg("blocks") = 200, py::arg("intercept") = py::none(),
           py::arg("weights") = py::none())
      .def("__len__", [](const LdScores& r) { return r.q.size(); })
      .def("__repr__", &LdScores::repr);

  m.def("ld_scores",
        [](const py::object& variants, int64_t window, const py::object& samples, const py::object& sites, const py::object& region, bool adjust) {
          ldscore_window_arg(window);
          auto store = store_from_python(variants);
          diploid_only(store->P, (size_t)store->S, "the LD scores take");
          vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
          return ld_scores_over_rows(rows_in_play(store, region), std::move(list), sites, window, adjust, "at least one sample is required for LD scores");
        },
        py::arg("variants"), py::arg("window") = 1000000, py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none(),
        py::arg("adjust") = true);
  population.def("ld_scores",
                 [](const Population& pop, int64_t window, const py::object& sites, bool adjust) {
                   ldscore_window_arg(window);
                   diploid_only(pop, "the LD scores take");
                   return ld_scores_over_rows(rows_in_play(pop), population_samples(pop), sites, window, adjust,
                                              "at least one sample with both haplotypes in the population is required for LD scores");
                 },
                 py::arg("window") = 1000000, py::arg("sites") = py::none(), py::arg("adjust") = true);
  m.def("ld_score_regression",
        [](const py::object& chi2, const py::object& scores, const py::object& n_samples, const py::object& m_sites, int64_t blocks, const py::object& intercept,
           const py::object& weights) {
          auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(scores);
          if (!arr || arr.ndim() != 1) value_error("scores must be a one-dimensional float array");
          const vector<double> l(arr.data(), arr.data() + arr.shape(0));
          const vector<double> y = f64_sites_arg(chi2, "chi2", l.size());
          return ld_score_regress(y, l, n_samples, m_sites, blocks, intercept, weights);
        },
        py::arg("chi2"), py::arg("scores"), py::arg("n_samples"), py::arg("m_sites") = py::none(), py::arg("blocks") = 200, py::arg("intercept") = py::none(),
        py::arg("weights") = py::none());
}
