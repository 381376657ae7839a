// pymodule_lmm.inc — ferromic.mixed_model_scan, Population.mixed_model_scan and the MixedModelScan result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows and sample rules it uses and pymodule_grm.inc whose GeneticRelationship it
// takes).  An addition to the reference's surface: it has no association scan; the definition is include/ferromic_hip.h's (fmh_lmm_null,
// fmh_lmm_projections, fmh_lmm_stats).  The null fit runs on the host, the projections come from the device row chunk by row chunk, and the
// statistics are computed from them on the host by the library as the chunks come down; the GIL is released around the C calls.

struct MixedModelScan {
  size_t rows = 0, n_phenotypes = 0;
  uint64_t n_samples = 0, df = 0;
  vector<double> beta, se, t, p;  // [rows][P]
  vector<uint32_t> n_called;      // [rows]
  vector<double> alt_frequency;   // [rows]
  vector<int64_t> positions;      // [rows] (empty when built from projections without them)
  vector<int64_t> kept, dropped;  // covariate column numbers
  vector<double> delta, sigma_g2, sigma_e2, heritability, log_likelihood;  // [P]
  vector<uint8_t> at_boundary;                                             // [P]
  vector<double> eigenvalues;                                              // [n]

  void reserve_rows(size_t r, size_t P) {
    rows = r; n_phenotypes = P;
    for (vector<double>* v : {&beta, &se, &t, &p}) v->assign(r * P, 0.0);
    n_called.assign(r, 0);
    alt_frequency.assign(r, 0.0);
  }
  py::array_t<double> table(const vector<double>& v) const {
    py::array_t<double> out({(py::ssize_t)rows, (py::ssize_t)n_phenotypes});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(double));
    return out;
  }
  // c and the alt allele frequency a / (2 c) (NaN where c = 0) of rows [at, at + count)
  void site_columns(size_t at, size_t count, const uint32_t* called, const uint32_t* allele_count) {
    for (size_t i = 0; i < count; ++i) {
      n_called[at + i] = called[i];
      alt_frequency[at + i] = called[i] ? (double)allele_count[i] / (2.0 * (double)called[i]) : std::numeric_limits<double>::quiet_NaN();
    }
  }
  string repr() const {
    return "MixedModelScan(samples=" + std::to_string(n_samples) + ", sites=" + std::to_string(rows) + ", phenotypes=" + std::to_string(n_phenotypes) +
           ", covariates=" + std::to_string(kept.size()) + ", df=" + std::to_string(df) + ")";
  }
};

using F64Array = py::array_t<double, py::array::c_style | py::array::forcecast>;

// the full eigenpairs of a relationship matrix [n][n] (host) through fmh_grm_eigen: values descending [n], vectors [n][n]
void lmm_eigen_of(int device, const vector<double>& matrix, size_t n, vector<double>& values, vector<double>& vectors) {
  for (double v : matrix)
    if (!std::isfinite(v)) value_error("the relationship matrix holds a value that is not finite");
  values.assign(n, 0.0);
  vectors.assign(n * n, 0.0);
  int status;
  {
    DevBuf d(device, matrix.size() * sizeof(double));
    py::gil_scoped_release nogil;
    status = fmh_copy_to_device(device, d.p, matrix.data(), matrix.size() * sizeof(double), nullptr);
    if (status == FMH_OK) status = fmh_grm_eigen(device, (double*)d.p, n, n, values.data(), vectors.data());
  }
  fmh_check(status);
}

// what the arguments say before any device is used: the phenotypes [n][P], the covariates, and the eigenpairs where they can be had without one
struct LmmInputs {
  size_t n = 0, P = 0, cin = 0;
  F64Array y, x;
  vector<double> matrix;           // the relationship matrix, empty when `eigen` was given
  vector<double> values, vectors;  // [n], [n][n]
  const GeneticRelationship* relationship = nullptr;  // its cache is asked when `eigen` was not given
};

LmmInputs lmm_inputs(const py::object& phenotypes, const py::object& relationship, const py::object& covariates, const py::object& eigen,
                     const vector<uint32_t>& samples) {
  LmmInputs in;
  const size_t n = in.n = samples.size();
  if (n == 0) value_error("at least one sample is required for a mixed-model scan");
  in.y = F64Array::ensure(phenotypes);
  if (!in.y || (in.y.ndim() != 1 && in.y.ndim() != 2)) value_error("phenotypes must be a numeric array [n] or [n][P]");
  if ((size_t)in.y.shape(0) != n) value_error("phenotypes has " + std::to_string(in.y.shape(0)) + " rows, expected one per selected sample (" + std::to_string(n) + ")");
  in.P = in.y.ndim() == 1 ? 1 : (size_t)in.y.shape(1);
  if (in.P == 0) value_error("at least one phenotype is required");
  if (!covariates.is_none()) {
    in.x = F64Array::ensure(covariates);
    if (!in.x || in.x.ndim() != 2) value_error("covariates must be a numeric array [n][c_in]");
    if ((size_t)in.x.shape(0) != n) value_error("covariates has " + std::to_string(in.x.shape(0)) + " rows, expected one per selected sample (" + std::to_string(n) + ")");
    in.cin = (size_t)in.x.shape(1);
  }
  if (in.cin + 2 > 64) value_error(std::to_string(in.cin) + " covariates: a phenotype takes c + 2 of the 64 coefficient rows of a call");
  for (py::ssize_t i = 0; i < in.y.size(); ++i)
    if (!std::isfinite(in.y.data()[i])) value_error("phenotypes holds a value that is not finite");
  for (py::ssize_t i = 0; i < (in.cin ? in.x.size() : 0); ++i)
    if (!std::isfinite(in.x.data()[i])) value_error("covariates holds a value that is not finite");
  if (py::isinstance<GeneticRelationship>(relationship)) {
    const GeneticRelationship& g = relationship.cast<const GeneticRelationship&>();
    if (g.samples != samples) value_error("the relationship matrix was computed for other samples than the scan's");
    in.relationship = &g;
  } else {
    auto a = F64Array::ensure(relationship);
    if (!a || a.ndim() != 2 || (size_t)a.shape(0) != n || (size_t)a.shape(1) != n)
      value_error("relationship must be a GeneticRelationship or a symmetric [n][n] array with one row per selected sample (" + std::to_string(n) + ")");
    in.matrix.assign(a.data(), a.data() + n * n);
    for (size_t i = 0; i < n; ++i)
      for (size_t j = 0; j < i; ++j)
        if (in.matrix[i * n + j] != in.matrix[j * n + i]) value_error("relationship is not symmetric");
  }
  if (!eigen.is_none()) {
    if (!py::isinstance<py::tuple>(eigen) && !py::isinstance<py::list>(eigen)) value_error("eigen must be (values [n], vectors [n][n])");
    const py::sequence pair = eigen.cast<py::sequence>();
    if (pair.size() != 2) value_error("eigen must be (values [n], vectors [n][n])");
    auto w = F64Array::ensure(pair[0]), u = F64Array::ensure(pair[1]);
    if (!w || !u || w.ndim() != 1 || u.ndim() != 2 || (size_t)w.shape(0) != n || (size_t)u.shape(0) != n || (size_t)u.shape(1) != n)
      value_error("eigen must be (values [n], vectors [n][n]) for the " + std::to_string(n) + " selected samples");
    in.values.assign(w.data(), w.data() + n);
    in.vectors.assign(u.data(), u.data() + n * n);
    for (double v : in.values)
      if (!std::isfinite(v)) value_error("eigen holds a value that is not finite");
    for (double v : in.vectors)
      if (!std::isfinite(v)) value_error("eigen holds a value that is not finite");
  }
  return in;
}

// the null fit of one batch of phenotypes
struct LmmBatch {
  size_t first = 0, P = 0, q = 0;
  vector<double> weights, linear, M, v, R;
};

MixedModelScan mixed_model_over_rows(const RowsInPlay& in_play, const vector<uint32_t>& samples, LmmInputs& in) {
  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  const size_t n = in.n, P = in.P, cin = in.cin;
  const int device = dm ? dm->device : (in.relationship ? in.relationship->device : current_device());
  if (in.values.empty()) {
    if (in.relationship) {
      in.relationship->eigen_pairs(in.values, in.vectors);
    } else {
      lmm_eigen_of(device, in.matrix, n, in.values, in.vectors);
    }
  }
  MixedModelScan out;
  out.n_samples = n;
  out.eigenvalues = in.values;
  out.positions = in_play.positions_copy();
  out.reserve_rows(dm ? rc : 0, P);
  for (vector<double>* v : {&out.delta, &out.sigma_g2, &out.sigma_e2, &out.heritability, &out.log_likelihood}) v->assign(P, 0.0);
  out.at_boundary.assign(P, 0);

  // ---- the null fits, in batches that keep P <= 16 and P (q + 1) <= 64 whatever the drop rule leaves of the covariates ----
  const size_t batch_size = std::min<size_t>(16, 64 / (cin + 2));
  vector<LmmBatch> batches;
  vector<uint8_t> dropped(std::max<size_t>(cin, 1), 0), reason(P, 0);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    for (size_t first = 0; first < P && status == FMH_OK; first += batch_size) {
      LmmBatch b;
      b.first = first;
      b.P = std::min(batch_size, P - first);
      const size_t qmax = cin + 1;
      vector<double> yb(n * b.P);
      for (size_t i = 0; i < n; ++i)
        for (size_t p = 0; p < b.P; ++p) yb[i * b.P + p] = in.y.data()[i * P + first + p];
      b.weights.assign(b.P * n, 0.0); b.linear.assign(b.P * (qmax + 1) * n, 0.0); b.M.assign(b.P * qmax * qmax, 0.0); b.v.assign(b.P * qmax, 0.0);
      b.R.assign(b.P, 0.0);
      fmh_lmm_null_out o{};
      o.h_delta = out.delta.data() + first; o.h_sigma_g2 = out.sigma_g2.data() + first; o.h_sigma_e2 = out.sigma_e2.data() + first;
      o.h_heritability = out.heritability.data() + first; o.h_log_likelihood = out.log_likelihood.data() + first;
      o.h_at_boundary = out.at_boundary.data() + first; o.h_reason = reason.data() + first;
      o.h_weights = b.weights.data(); o.h_linear = b.linear.data(); o.h_m = b.M.data(); o.h_v = b.v.data(); o.h_r = b.R.data();
      status = fmh_lmm_null(in.values.data(), in.vectors.data(), yb.data(), cin ? in.x.data() : nullptr, n, b.P, cin, nullptr, &b.q, cin ? dropped.data() : nullptr, &o);
      batches.push_back(std::move(b));
    }
  }
  fmh_check_args(status);  // too few samples for the design matrix: the caller's arguments
  const size_t q = batches.front().q;
  out.df = n - q - 1;
  for (size_t j = 0; j < cin; ++j) (dropped[j] ? out.dropped : out.kept).push_back((int64_t)j);
  if (!dm || rc == 0) return out;

  // ---- the projections, batch by batch and row chunk by row chunk ----
  // (the buffers are sized for the first batch, the largest)
  const size_t widest = batches.front().P * (q + 2);
  const size_t chunk_rows = chunk_rows_under("FMH_ASSOC_BUDGET_BYTES", rc, widest * sizeof(double));
  DevBuf d_basis(device, n * n * sizeof(double)), d_coef(device, widest * n * sizeof(double)), d_out(device, chunk_rows * widest * sizeof(double));
  vector<uint32_t> called, allele_count;
  {
    py::gil_scoped_release nogil;
    status = fmh_copy_to_device(device, d_basis.p, in.vectors.data(), n * n * sizeof(double), nullptr);
    for (const LmmBatch& b : batches) {
      if (status != FMH_OK) break;
      const size_t L = b.P * (q + 1);
      double *d_weights = (double*)d_coef.p, *d_linear = d_weights + b.P * n, *d_quad = (double*)d_out.p, *d_lin = d_quad + chunk_rows * b.P;
      status = fmh_copy_to_device(device, d_weights, b.weights.data(), b.P * n * sizeof(double), nullptr);
      if (status == FMH_OK) status = fmh_copy_to_device(device, d_linear, b.linear.data(), L * n * sizeof(double), nullptr);
      vector<double> quad(chunk_rows * b.P), lin(chunk_rows * L), stat[4];
      for (vector<double>& s : stat) s.assign(chunk_rows * b.P, 0.0);
      called.assign(chunk_rows, 0);
      allele_count.assign(chunk_rows, 0);
      for (size_t at = 0; at < rc && status == FMH_OK; at += chunk_rows) {
        const size_t count = std::min(chunk_rows, rc - at);
        status = fmh_lmm_projections(dm->h, samples.data(), n, r0 + at, count, (const double*)d_basis.p, n, d_weights, b.P, d_linear, L, d_quad, d_lin,
                                     called.data(), allele_count.data(), nullptr);
        if (status == FMH_OK) status = fmh_copy_to_host(device, quad.data(), d_quad, count * b.P * sizeof(double), nullptr);
        if (status == FMH_OK) status = fmh_copy_to_host(device, lin.data(), d_lin, count * L * sizeof(double), nullptr);
        if (status == FMH_OK)
          status = fmh_lmm_stats(quad.data(), lin.data(), called.data(), allele_count.data(), count, b.M.data(), b.v.data(), b.R.data(), n, q, b.P,
                                 stat[0].data(), stat[1].data(), stat[2].data(), stat[3].data());
        if (status != FMH_OK) break;
        vector<double>* columns[4] = {&out.beta, &out.se, &out.t, &out.p};
        for (int s = 0; s < 4; ++s)
          for (size_t i = 0; i < count; ++i)
            for (size_t p = 0; p < b.P; ++p) (*columns[s])[(at + i) * P + b.first + p] = stat[s][i * b.P + p];
        out.site_columns(at, count, called.data(), allele_count.data());
      }
    }
  }
  fmh_check(status);
  return out;
}

MixedModelScan mixed_model_scan(const py::object& variants, const py::object& phenotypes, const py::object& relationship, const py::object& covariates,
                                const py::object& samples, const py::object& region, const py::object& eigen) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "the mixed-model scan takes");
  const vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  LmmInputs in = lmm_inputs(phenotypes, relationship, covariates, eigen, list);
  return mixed_model_over_rows(rows_in_play(store, region), list, in);
}

MixedModelScan population_mixed_model_scan(const Population& pop, const py::object& phenotypes, const py::object& relationship, const py::object& covariates,
                                           const py::object& eigen) {
  diploid_only(pop, "the mixed-model scan takes");
  const vector<uint32_t> list = population_samples(pop);
  LmmInputs in = lmm_inputs(phenotypes, relationship, covariates, eigen, list);
  return mixed_model_over_rows(rows_in_play(pop), list, in);
}

// A result from projections that were computed before (no device): quad [rows][P], lin [rows][P (q + 1)], the counts, and the null fit's
// M [P][q][q], v [P][q], R [P].
MixedModelScan mixed_model_from_projections(const py::object& quad, const py::object& lin, const py::object& called, const py::object& allele_count,
                                            const py::object& m, const py::object& v, const py::object& r, uint64_t n_samples, const py::object& positions,
                                            const py::object& delta, const py::object& covariates_kept, const py::object& covariates_dropped,
                                            const py::object& eigenvalues) {
  MixedModelScan out;
  const vector<uint32_t> c = vector_arg<uint32_t>(called, "called", 0, false), a = vector_arg<uint32_t>(allele_count, "allele_count", c.size(), true);
  auto rv = F64Array::ensure(r), vv = F64Array::ensure(v), mv = F64Array::ensure(m), qv = F64Array::ensure(quad), lv = F64Array::ensure(lin);
  if (!rv || rv.ndim() != 1 || rv.shape(0) < 1) value_error("r must be a one-dimensional array with one entry per phenotype");
  const size_t rows = c.size(), P = (size_t)rv.shape(0);
  if (!vv || vv.ndim() != 2 || (size_t)vv.shape(0) != P || vv.shape(1) < 1) value_error("v must be [P][q]");
  const size_t q = (size_t)vv.shape(1);
  if (!mv || (size_t)mv.size() != P * q * q) value_error("m must hold [P][q][q] = " + std::to_string(P * q * q) + " values");
  if (!qv || (size_t)qv.size() != rows * P) value_error("quad must hold [rows][P] = " + std::to_string(rows * P) + " values");
  if (!lv || (size_t)lv.size() != rows * P * (q + 1)) value_error("lin must hold [rows][P (q + 1)] = " + std::to_string(rows * P * (q + 1)) + " values");
  if (!positions.is_none()) out.positions = vector_arg<int64_t>(positions, "positions", rows, true);
  if (!covariates_kept.is_none()) out.kept = vector_arg<int64_t>(covariates_kept, "covariates_kept", q - 1, true);
  if (!covariates_dropped.is_none()) out.dropped = vector_arg<int64_t>(covariates_dropped, "covariates_dropped", 0, false);
  if (!delta.is_none()) {
    auto dv = F64Array::ensure(delta);
    if (!dv || (size_t)dv.size() != P) value_error("delta must hold one value per phenotype");
    out.delta.assign(dv.data(), dv.data() + P);
    for (double d : out.delta) { out.heritability.push_back(1.0 / (1.0 + d)); }
  }
  if (!eigenvalues.is_none()) {
    auto ev = F64Array::ensure(eigenvalues);
    if (!ev || ev.ndim() != 1) value_error("eigenvalues must be a one-dimensional array");
    out.eigenvalues.assign(ev.data(), ev.data() + ev.size());
  }
  out.n_samples = n_samples;
  out.reserve_rows(rows, P);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_lmm_stats(qv.data(), lv.data(), c.data(), a.data(), rows, mv.data(), vv.data(), rv.data(), n_samples, q, P, out.beta.data(), out.se.data(),
                           out.t.data(), out.p.data());
  }
  fmh_check_args(status);
  out.df = n_samples - q - 1;
  out.site_columns(0, rows, c.data(), a.data());
  return out;
}

void bind_lmm(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<MixedModelScan>(m, "MixedModelScan")
      .def_static("from_projections", &mixed_model_from_projections, py::arg("quad"), py::arg("lin"), py::arg("called"), py::arg("allele_count"), py::arg("m"),
                  py::arg("v"), py::arg("r"), py::arg("n_samples"), py::arg("positions") = py::none(), py::arg("delta") = py::none(),
                  py::arg("covariates_kept") = py::none(), py::arg("covariates_dropped") = py::none(), py::arg("eigenvalues") = py::none())
      .def_property_readonly("beta", [](const MixedModelScan& a) { return a.table(a.beta); })
      .def_property_readonly("se", [](const MixedModelScan& a) { return a.table(a.se); })
      .def_property_readonly("t", [](const MixedModelScan& a) { return a.table(a.t); })
      .def_property_readonly("p", [](const MixedModelScan& a) { return a.table(a.p); })
      .def_property_readonly("n_called", [](const MixedModelScan& a) { return array_of(a.n_called); })
      .def_property_readonly("alt_frequency", [](const MixedModelScan& a) { return array_of(a.alt_frequency); })
      .def_property_readonly("positions", [](const MixedModelScan& a) { return array_of(a.positions); })
      .def_property_readonly("df", [](const MixedModelScan& a) { return a.df; })
      .def_property_readonly("delta", [](const MixedModelScan& a) { return array_of(a.delta); })
      .def_property_readonly("sigma_g2", [](const MixedModelScan& a) { return array_of(a.sigma_g2); })
      .def_property_readonly("sigma_e2", [](const MixedModelScan& a) { return array_of(a.sigma_e2); })
      .def_property_readonly("heritability", [](const MixedModelScan& a) { return array_of(a.heritability); })
      .def_property_readonly("log_likelihood", [](const MixedModelScan& a) { return array_of(a.log_likelihood); })
      .def_property_readonly("at_boundary", [](const MixedModelScan& a) {
        py::array_t<bool> out((py::ssize_t)a.at_boundary.size());
        for (size_t i = 0; i < a.at_boundary.size(); ++i) out.mutable_data()[i] = a.at_boundary[i] != 0;
        return out;
      })
      .def_property_readonly("covariates_kept", [](const MixedModelScan& a) { return array_of(a.kept); })
      .def_property_readonly("covariates_dropped", [](const MixedModelScan& a) { return array_of(a.dropped); })
      .def_property_readonly("eigenvalues", [](const MixedModelScan& a) { return array_of(a.eigenvalues); })
      .def("__len__", [](const MixedModelScan& a) { return a.rows; })
      .def("__repr__", &MixedModelScan::repr);
  m.def("mixed_model_scan", &mixed_model_scan, py::arg("variants"), py::arg("phenotypes"), py::arg("relationship"), py::arg("covariates") = py::none(),
        py::arg("samples") = py::none(), py::arg("region") = py::none(), py::arg("eigen") = py::none());
  population.def("mixed_model_scan", &population_mixed_model_scan, py::arg("phenotypes"), py::arg("relationship"), py::arg("covariates") = py::none(),
                 py::arg("eigen") = py::none());
}
