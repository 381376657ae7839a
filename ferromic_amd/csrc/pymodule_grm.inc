// pymodule_grm.inc — ferromic.grm, Population.grm and the GeneticRelationship / GenotypePCA results (included inside pymodule_stats.inc's
// namespace, after the argument handling the statistics share).  An addition to the reference's surface: its PCA is the haplotype PCA; the
// definition is include/ferromic_hip.h's (fmh_grm, fmh_grm_values, fmh_grm_finish, fmh_grm_eigen).  The products and the pair counts come from
// the device; frequency and the matrix are computed from them on the host by the library; the GIL is released around the C calls.

struct GenotypePCA {
  vector<uint32_t> samples;
  size_t k = 0;
  vector<double> eigenvalues, eigenvectors, explained;  // [k], [n][k], [k]
  string repr() const { return "GenotypePCA(samples=" + std::to_string(samples.size()) + ", components=" + std::to_string(k) + ")"; }
};

struct GeneticRelationship {
  vector<uint32_t> samples;   // sample numbers, ascending
  vector<int64_t> sites;      // the kept rows, as indices into the rows in play
  vector<uint32_t> called, allele_count;  // per kept row
  vector<uint8_t> usable;
  vector<double> frequency;
  vector<double> products, matrix;  // S, A: [n][n]
  vector<uint64_t> pair_sites;      // N: [n][n], empty unless denominator="pairs"
  fmh_grm_params params{FMH_GRM_STANDARDIZED, FMH_GRM_SITES};
  uint64_t n_usable = 0;
  double scale = 0.0;
  int device = 0;
  mutable vector<double> eigen_values, eigen_vectors;  // every eigenpair of A ([n], [n][n]), computed when first asked (eigen())

  size_t n() const { return samples.size(); }
  template <class T> py::array_t<T> square(const vector<T>& v) const {
    py::array_t<T> out(std::vector<py::ssize_t>{(py::ssize_t)n(), (py::ssize_t)n()});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(T));
    return out;
  }
  py::array_t<double> inbreeding() const {
    py::array_t<double> out((py::ssize_t)n());
    for (size_t i = 0; i < n(); ++i) out.mutable_data()[i] = matrix[i * n() + i] - 1.0;
    return out;
  }
  GenotypePCA pca(int64_t n_components) const {
    if (n_components < 1) value_error("n_components must be at least 1");
    for (double v : matrix)
      if (v != v) value_error("the relationship matrix holds a NaN: with denominator=\"pairs\" a pair of samples without a jointly called usable site has no value");
    GenotypePCA out;
    out.samples = samples;
    out.k = std::min<size_t>((size_t)n_components, n());
    out.eigenvalues.assign(out.k, 0.0);
    out.eigenvectors.assign(n() * out.k, 0.0);
    int status;
    {
      DevBuf d(device, matrix.size() * sizeof(double));
      py::gil_scoped_release nogil;
      status = fmh_copy_to_device(device, d.p, matrix.data(), matrix.size() * sizeof(double), nullptr);
      if (status == FMH_OK) status = fmh_grm_eigen(device, (double*)d.p, n(), out.k, out.eigenvalues.data(), out.eigenvectors.data());
    }
    fmh_check(status);
    double trace = 0.0;
    for (size_t i = 0; i < n(); ++i) trace += matrix[i * n() + i];
    for (double v : out.eigenvalues) out.explained.push_back(v / trace);
    return out;
  }
  // every eigenpair of A through fmh_grm_eigen, descending: what the mixed-model scan rotates by.  Computed once and kept.
  void eigen_pairs(vector<double>& values, vector<double>& vectors) const {
    if (eigen_values.empty()) {
      for (double v : matrix)
        if (v != v) value_error("the relationship matrix holds a NaN: with denominator=\"pairs\" a pair of samples without a jointly called usable site has no value");
      vector<double> w(n(), 0.0), u(n() * n(), 0.0);
      int status;
      {
        DevBuf d(device, matrix.size() * sizeof(double));
        py::gil_scoped_release nogil;
        status = fmh_copy_to_device(device, d.p, matrix.data(), matrix.size() * sizeof(double), nullptr);
        if (status == FMH_OK) status = fmh_grm_eigen(device, (double*)d.p, n(), n(), w.data(), u.data());
      }
      fmh_check(status);
      eigen_values = std::move(w);
      eigen_vectors = std::move(u);
    }
    values = eigen_values;
    vectors = eigen_vectors;
  }
  string repr() const {
    return "GeneticRelationship(samples=" + std::to_string(n()) + ", sites=" + std::to_string(sites.size()) + ", usable=" + std::to_string(n_usable) + ")";
  }
};

// method and denominator as the Python surface spells them; refused before anything is uploaded
fmh_grm_params grm_params_arg(const string& method, const string& denominator) {
  fmh_grm_params P{};
  if (method == "standardized") P.method = FMH_GRM_STANDARDIZED;
  else if (method == "centered") P.method = FMH_GRM_CENTERED;
  else value_error("method must be \"standardized\" or \"centered\", got \"" + method + "\"");
  if (denominator == "sites") P.denominator = FMH_GRM_SITES;
  else if (denominator == "pairs") P.denominator = FMH_GRM_PAIRS;
  else value_error("denominator must be \"sites\" or \"pairs\", got \"" + denominator + "\"");
  if (P.denominator == FMH_GRM_PAIRS && P.method != FMH_GRM_STANDARDIZED) value_error("denominator=\"pairs\" takes method=\"standardized\" only");
  return P;
}

GeneticRelationship grm_over_rows(const ResidentRows& rows, vector<uint32_t> samples, const py::object& sites, const fmh_grm_params& P) {
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  GeneticRelationship out;
  out.samples = std::move(samples);
  out.params = P;
  const size_t n = out.n();
  if (n == 0) value_error("at least one sample is required for a relationship matrix");
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  for (size_t i = 0; i < rc; ++i)
    if (!masked || keep[i]) out.sites.push_back((int64_t)i);
  const size_t total = n * n, kept = out.sites.size();
  const bool pairs = P.denominator == FMH_GRM_PAIRS;
  out.products.assign(total, 0.0);
  out.matrix.assign(total, 0.0);
  if (pairs) out.pair_sites.assign(total, 0);
  out.called.assign(std::max<size_t>(rc, 1), 0);
  out.allele_count.assign(std::max<size_t>(rc, 1), 0);
  out.usable.assign(std::max<size_t>(rc, 1), 0);
  out.frequency.assign(kept, 0.0);
  out.device = dm ? dm->device : current_device();
  int status = FMH_OK;
  if (dm && rc != 0) {
    DevBuf d(dm->device, total * sizeof(double) + (pairs ? total * sizeof(uint64_t) : 0));
    fmh_grm_out bufs{};
    bufs.d_products = (double*)d.p;
    bufs.d_pair_sites = pairs ? (unsigned long long*)((double*)d.p + total) : nullptr;
    bufs.h_called = out.called.data(); bufs.h_allele_count = out.allele_count.data(); bufs.h_usable = out.usable.data();
    bufs.h_usable_rows = &out.n_usable; bufs.h_scale = &out.scale;
    py::gil_scoped_release nogil;
    status = fmh_device_zero(dm->device, d.p, total * sizeof(double) + (pairs ? total * sizeof(uint64_t) : 0), nullptr);
    if (status == FMH_OK) status = fmh_grm(dm->h, out.samples.data(), n, r0, rc, masked ? keep.data() : nullptr, &P, &bufs, nullptr, nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm->device, out.products.data(), bufs.d_products, total * sizeof(double), nullptr);
    if (status == FMH_OK && pairs) status = fmh_copy_to_host(dm->device, out.pair_sites.data(), bufs.d_pair_sites, total * sizeof(uint64_t), nullptr);
  }
  fmh_check(status);
  out.called.resize(kept); out.allele_count.resize(kept); out.usable.resize(kept);
  {
    py::gil_scoped_release nogil;
    status = fmh_grm_values(out.called.data(), out.allele_count.data(), kept, P.method, nullptr, out.frequency.data(), nullptr, nullptr, nullptr);
    if (status == FMH_OK) status = fmh_grm_finish(out.products.data(), pairs ? out.pair_sites.data() : nullptr, n, &P, out.n_usable, out.scale, out.matrix.data());
  }
  fmh_check(status);
  return out;
}

GeneticRelationship grm(const py::object& variants, const py::object& samples, const py::object& sites, const py::object& region, const string& method,
                        const string& denominator) {
  const fmh_grm_params P = grm_params_arg(method, denominator);
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "the relationship matrix takes");
  vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  if (list.empty()) value_error("at least one sample is required for a relationship matrix");
  return grm_over_rows(rows_in_play(store, region).resident(), std::move(list), sites, P);
}

GeneticRelationship population_grm(const Population& pop, const py::object& sites, const string& method, const string& denominator) {
  const fmh_grm_params P = grm_params_arg(method, denominator);
  diploid_only(pop, "the relationship matrix takes");
  vector<uint32_t> list = population_samples(pop);
  if (list.empty()) value_error("at least one sample is required for a relationship matrix");
  return grm_over_rows(rows_in_play(pop).resident(), std::move(list), sites, P);
}

template <class Class> void bind_grm(py::module_& m, Class& population) {
  py::class_<GenotypePCA>(m, "GenotypePCA")
      .def_property_readonly("samples", [](const GenotypePCA& p) {
        py::array_t<int64_t> out((py::ssize_t)p.samples.size());
        for (size_t i = 0; i < p.samples.size(); ++i) out.mutable_data()[i] = p.samples[i];
        return out;
      })
      .def_property_readonly("eigenvalues", [](const GenotypePCA& p) { return array_of(p.eigenvalues); })
      .def_property_readonly("explained", [](const GenotypePCA& p) { return array_of(p.explained); })
      .def_property_readonly("eigenvectors", [](const GenotypePCA& p) {
        py::array_t<double> out(std::vector<py::ssize_t>{(py::ssize_t)p.samples.size(), (py::ssize_t)p.k});
        if (!p.eigenvectors.empty()) memcpy(out.mutable_data(), p.eigenvectors.data(), p.eigenvectors.size() * sizeof(double));
        return out;
      })
      .def("__repr__", &GenotypePCA::repr);
  py::class_<GeneticRelationship>(m, "GeneticRelationship")
      .def_property_readonly("samples", [](const GeneticRelationship& g) {
        py::array_t<int64_t> out((py::ssize_t)g.n());
        for (size_t i = 0; i < g.n(); ++i) out.mutable_data()[i] = g.samples[i];
        return out;
      })
      .def_property_readonly("sites", [](const GeneticRelationship& g) { return array_of(g.sites); })
      .def_property_readonly("usable", [](const GeneticRelationship& g) {
        py::array_t<bool> out((py::ssize_t)g.usable.size());
        for (size_t i = 0; i < g.usable.size(); ++i) out.mutable_data()[i] = g.usable[i] != 0;
        return out;
      })
      .def_property_readonly("n_usable", [](const GeneticRelationship& g) { return g.n_usable; })
      .def_property_readonly("called", [](const GeneticRelationship& g) { return array_of(g.called); })
      .def_property_readonly("allele_count", [](const GeneticRelationship& g) { return array_of(g.allele_count); })
      .def_property_readonly("frequency", [](const GeneticRelationship& g) { return array_of(g.frequency); })
      .def_property_readonly("products", [](const GeneticRelationship& g) { return g.square(g.products); })
      .def_property_readonly("pair_sites", [](const GeneticRelationship& g) -> py::object {
        return g.params.denominator == FMH_GRM_PAIRS ? py::object(g.square(g.pair_sites)) : py::object(py::none());
      })
      .def_property_readonly("matrix", [](const GeneticRelationship& g) { return g.square(g.matrix); })
      .def_property_readonly("scale", [](const GeneticRelationship& g) { return g.scale; })
      .def("inbreeding", &GeneticRelationship::inbreeding)
      .def("pca", &GeneticRelationship::pca, py::arg("n_components") = 10)
      .def("eigen", [](const GeneticRelationship& g) {
        vector<double> values, vectors;
        g.eigen_pairs(values, vectors);
        return py::make_tuple(array_of(values), g.square(vectors));
      })
      .def("__repr__", &GeneticRelationship::repr);
  m.def("grm", &grm, py::arg("variants"), py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none(),
        py::arg("method") = "standardized", py::arg("denominator") = "sites");
  population.def("grm", &population_grm, py::arg("sites") = py::none(), py::arg("method") = "standardized", py::arg("denominator") = "sites");
}
