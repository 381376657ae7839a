// pymodule_assoc.inc — ferromic.association_scan, Population.association_scan and the AssociationScan result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample rules and chunk tracks it uses).  An addition to the reference's
// surface: it has no association scan; the definition is include/ferromic_hip.h's (fmh_assoc_prepare, fmh_assoc_sums, fmh_assoc_stats).
// The exact sums come from the device, row chunk by row chunk; the statistics are computed from them on the host by the library as the
// chunks come down; the GIL is released around the C calls.

struct AssociationScan {
  size_t rows = 0, n_phenotypes = 0;
  uint64_t n_samples = 0, df = 0;
  vector<double> beta, se, t, p;  // [rows][P]
  vector<uint32_t> n_called;      // [rows]
  vector<double> alt_frequency;   // [rows]
  vector<int64_t> positions;      // [rows] (empty when built from sums without them)
  vector<int64_t> kept, dropped;  // covariate column numbers

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
  string repr() const {
    return "AssociationScan(samples=" + std::to_string(n_samples) + ", sites=" + std::to_string(rows) + ", phenotypes=" + std::to_string(n_phenotypes) +
           ", covariates=" + std::to_string(kept.size()) + ", df=" + std::to_string(df) + ")";
  }
};

// what fmh_assoc_prepare made of the phenotypes and covariates
struct AssocModel {
  size_t n = 0, c = 0, P = 0;
  vector<int32_t> values, exponent;
  vector<long long> total;
  vector<double> yy;
  vector<int64_t> kept, dropped;
};

// [n] or [n][P] / [n][c_in] f64, in the order of the selected samples; every argument error before any device use
AssocModel assoc_model(const py::object& phenotypes, const py::object& covariates, size_t n) {
  auto y = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(phenotypes);
  if (!y || (y.ndim() != 1 && y.ndim() != 2)) value_error("phenotypes must be a numeric array [n] or [n][P]");
  if ((size_t)y.shape(0) != n) value_error("phenotypes has " + std::to_string(y.shape(0)) + " rows, expected one per selected sample (" + std::to_string(n) + ")");
  AssocModel out;
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
  if (n == 0) value_error("at least one sample is required for an association scan");
  out.values.assign(n * (cin + out.P), 0);
  out.exponent.assign(cin + out.P, 0);
  out.total.assign(cin + out.P, 0);
  out.yy.assign(out.P, 0.0);
  vector<uint8_t> dropped(cin, 0);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_assoc_prepare(y.data(), cin ? x.data() : nullptr, n, out.P, cin, out.values.data(), out.exponent.data(), out.total.data(), out.yy.data(),
                               &out.c, cin ? dropped.data() : nullptr);
  }
  fmh_check_args(status);  // a non-finite input, too few samples, too many columns: the caller's arguments
  for (size_t j = 0; j < cin; ++j) (dropped[j] ? out.dropped : out.kept).push_back((int64_t)j);
  return out;
}

// N and the alt allele frequency of rows [at, at + count) from the tracks; a library status (callable with the GIL released)
int assoc_site_columns(AssociationScan& out, size_t at, size_t count, const uint32_t* ref, const uint32_t* het, const uint32_t* alt) {
  for (size_t i = 0; i < count; ++i) out.n_called[at + i] = ref[i] + het[i] + alt[i];
  const fmh_genotype_site_stats_out site{nullptr, out.alt_frequency.data() + at, nullptr, nullptr, nullptr};
  return fmh_genotype_site_stats(ref, het, alt, count, out.n_samples, &site);
}

// A result from sums that were computed before (no device).
AssociationScan association_from_sums(const py::object& dosage_sum, const py::object& called_sum, const py::object& hom_ref, const py::object& het,
                                      const py::object& hom_alt, const py::object& total, const py::object& exponent, const py::object& yy,
                                      uint64_t n_samples, size_t n_basis, const py::object& positions, const py::object& covariates_kept,
                                      const py::object& covariates_dropped) {
  AssociationScan out;
  const vector<uint32_t> ref = vector_arg<uint32_t>(hom_ref, "hom_ref", 0, false);
  const vector<uint32_t> h = vector_arg<uint32_t>(het, "het", ref.size(), true), alt = vector_arg<uint32_t>(hom_alt, "hom_alt", ref.size(), true);
  auto yv = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(yy);
  if (!yv || yv.ndim() != 1 || yv.shape(0) < 1) value_error("yy must be a one-dimensional array with one entry per phenotype");
  const size_t rows = ref.size(), P = (size_t)yv.shape(0), K = n_basis + P;
  const vector<long long> tot = vector_arg<long long>(total, "total", K, true);
  const vector<int32_t> e = vector_arg<int32_t>(exponent, "exponent", K, true);
  const string shape = "hold [rows][c + P] = " + std::to_string(rows * K) + " integers";
  const vector<long long> S = i64_table_arg(dosage_sum, "dosage_sum", rows * K, shape), C = i64_table_arg(called_sum, "called_sum", rows * K, shape);
  if (!positions.is_none()) out.positions = vector_arg<int64_t>(positions, "positions", rows, true);
  if (!covariates_kept.is_none()) out.kept = vector_arg<int64_t>(covariates_kept, "covariates_kept", n_basis, true);
  if (!covariates_dropped.is_none()) out.dropped = vector_arg<int64_t>(covariates_dropped, "covariates_dropped", 0, false);
  out.n_samples = n_samples;
  out.reserve_rows(rows, P);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_assoc_stats(S.data(), C.data(), ref.data(), h.data(), alt.data(), rows, tot.data(), e.data(), yv.data(), n_samples, n_basis, P,
                             out.beta.data(), out.se.data(), out.t.data(), out.p.data());
  }
  fmh_check_args(status);
  out.df = n_samples - n_basis - 2;
  fmh_check(assoc_site_columns(out, 0, rows, ref.data(), h.data(), alt.data()));
  return out;
}

AssociationScan association_over_rows(const RowsInPlay& in_play, const vector<uint32_t>& samples, const AssocModel& model) {
  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  AssociationScan out;
  const size_t n = model.n, c = model.c, P = model.P, K = c + P;
  out.n_samples = n;
  out.df = n - c - 2;
  out.kept = model.kept;
  out.dropped = model.dropped;
  out.positions = in_play.positions_copy();
  out.reserve_rows(dm ? rc : 0, P);
  if (!dm || rc == 0) return out;
  const size_t chunk_rows = chunk_rows_under("FMH_ASSOC_BUDGET_BYTES", rc, 2 * K * sizeof(long long));
  DevBuf d_sums(dm->device, 2 * chunk_rows * K * sizeof(long long));
  long long* d_s = (long long*)d_sums.p;
  long long* d_c = d_s + chunk_rows * K;
  ChunkTracks tracks(dm->device, chunk_rows);
  vector<long long> S(chunk_rows * K), C(chunk_rows * K);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    const int dev = dm->device;
    for (size_t at = 0; at < rc && status == FMH_OK; at += chunk_rows) {
      const size_t count = std::min(chunk_rows, rc - at);
      status = fmh_genotype_counts(dm->h, samples.data(), n, r0 + at, count, nullptr, nullptr, &tracks.site, nullptr, nullptr, nullptr);
      if (status == FMH_OK) status = fmh_assoc_sums(dm->h, samples.data(), n, r0 + at, count, model.values.data(), K, d_s, d_c, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, S.data(), d_s, count * K * sizeof(long long), nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, C.data(), d_c, count * K * sizeof(long long), nullptr);
      if (status == FMH_OK) status = tracks.download();
      const uint32_t *ref = tracks.ref(), *het = tracks.het(), *alt = tracks.alt();
      if (status == FMH_OK)
        status = fmh_assoc_stats(S.data(), C.data(), ref, het, alt, count, model.total.data(), model.exponent.data(), model.yy.data(), n, c, P,
                                 out.beta.data() + at * P, out.se.data() + at * P, out.t.data() + at * P, out.p.data() + at * P);
      if (status == FMH_OK) status = assoc_site_columns(out, at, count, ref, het, alt);
    }
  }
  fmh_check(status);
  return out;
}

AssociationScan association_scan(const py::object& variants, const py::object& phenotypes, const py::object& covariates, const py::object& samples,
                                 const py::object& region) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "the association scan takes");
  const vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  const AssocModel model = assoc_model(phenotypes, covariates, list.size());
  return association_over_rows(rows_in_play(store, region), list, model);
}

AssociationScan population_association_scan(const Population& pop, const py::object& phenotypes, const py::object& covariates) {
  diploid_only(pop, "the association scan takes");
  const vector<uint32_t> list = population_samples(pop);
  const AssocModel model = assoc_model(phenotypes, covariates, list.size());
  return association_over_rows(rows_in_play(pop), list, model);
}

void bind_assoc(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<AssociationScan>(m, "AssociationScan")
      .def_static("from_sums", &association_from_sums, py::arg("dosage_sum"), py::arg("called_sum"), py::arg("hom_ref"), py::arg("het"),
                  py::arg("hom_alt"), py::arg("total"), py::arg("exponent"), py::arg("yy"), py::arg("n_samples"), py::arg("n_basis"),
                  py::arg("positions") = py::none(), py::arg("covariates_kept") = py::none(), py::arg("covariates_dropped") = py::none())
      .def_property_readonly("beta", [](const AssociationScan& a) { return a.table(a.beta); })
      .def_property_readonly("se", [](const AssociationScan& a) { return a.table(a.se); })
      .def_property_readonly("t", [](const AssociationScan& a) { return a.table(a.t); })
      .def_property_readonly("p", [](const AssociationScan& a) { return a.table(a.p); })
      .def_property_readonly("n_called", [](const AssociationScan& a) { return array_of(a.n_called); })
      .def_property_readonly("alt_frequency", [](const AssociationScan& a) { return array_of(a.alt_frequency); })
      .def_property_readonly("positions", [](const AssociationScan& a) { return array_of(a.positions); })
      .def_property_readonly("df", [](const AssociationScan& a) { return a.df; })
      .def_property_readonly("covariates_kept", [](const AssociationScan& a) { return array_of(a.kept); })
      .def_property_readonly("covariates_dropped", [](const AssociationScan& a) { return array_of(a.dropped); })
      .def("__len__", [](const AssociationScan& a) { return a.rows; })
      .def("__repr__", &AssociationScan::repr);
  m.def("association_scan", &association_scan, py::arg("variants"), py::arg("phenotypes"), py::arg("covariates") = py::none(),
        py::arg("samples") = py::none(), py::arg("region") = py::none());
  population.def("association_scan", &population_association_scan, py::arg("phenotypes"), py::arg("covariates") = py::none());
}
