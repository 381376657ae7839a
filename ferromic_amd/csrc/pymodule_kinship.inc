// pymodule_kinship.inc — ferromic.kinship, Population.kinship and the Kinship result (included inside pymodule_stats.inc's namespace, after
// the argument handling the statistics share).  An addition to the reference's surface: it has no relatedness code; the definition is
// include/ferromic_hip.h's (fmh_kinship_counts, fmh_kinship_stats, fmh_kinship_unrelated).  The four tables are exact integers from the
// device; kinship and IBS distance are computed from them on the host by the library; the GIL is released around the C calls.

struct Kinship {
  vector<uint32_t> samples;   // sample numbers, ascending
  vector<int64_t> sites;      // the kept rows, as indices into the rows in play
  vector<uint64_t> both, het_het, ibs0, het_hom;  // [n][n]
  vector<double> phi, ibs_distance;

  size_t n() const { return samples.size(); }
  template <class T> py::array_t<T> square(const vector<T>& v) const {
    py::array_t<T> out(std::vector<py::ssize_t>{(py::ssize_t)n(), (py::ssize_t)n()});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(T));
    return out;
  }
  py::array_t<bool> unrelated(double threshold) const {
    vector<uint8_t> keep(n(), 1);
    int status;
    {
      py::gil_scoped_release nogil;
      status = fmh_kinship_unrelated(phi.data(), n(), threshold, keep.data());
    }
    fmh_check(status);
    py::array_t<bool> out((py::ssize_t)n());
    bool* o = out.mutable_data();
    for (size_t i = 0; i < n(); ++i) o[i] = keep[i] != 0;
    return out;
  }
  string repr() const { return "Kinship(samples=" + std::to_string(n()) + ", sites=" + std::to_string(sites.size()) + ")"; }
};

Kinship kinship_over_rows(const ResidentRows& rows, vector<uint32_t> samples, const py::object& sites) {
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  Kinship out;
  out.samples = std::move(samples);
  const size_t n = out.n();
  if (n == 0) value_error("at least one sample is required for kinship");
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  for (size_t i = 0; i < rc; ++i)
    if (!masked || keep[i]) out.sites.push_back((int64_t)i);
  const size_t total = n * n;
  out.both.assign(total, 0); out.het_het.assign(total, 0); out.ibs0.assign(total, 0); out.het_hom.assign(total, 0);
  out.phi.assign(total, 0.0); out.ibs_distance.assign(total, 0.0);
  int status = FMH_OK;
  if (dm && rc != 0) {
    DevBuf d(dm->device, 4 * total * sizeof(uint64_t));
    unsigned long long* base = (unsigned long long*)d.p;
    fmh_kinship_out bufs{base, base + total, base + 2 * total, base + 3 * total};
    py::gil_scoped_release nogil;
    status = fmh_device_zero(dm->device, d.p, 4 * total * sizeof(uint64_t), nullptr);
    if (status == FMH_OK) status = fmh_kinship_counts(dm->h, out.samples.data(), n, r0, rc, masked ? keep.data() : nullptr, &bufs, nullptr, nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm->device, out.both.data(), bufs.d_both, total * sizeof(uint64_t), nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm->device, out.het_het.data(), bufs.d_het_het, total * sizeof(uint64_t), nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm->device, out.ibs0.data(), bufs.d_ibs0, total * sizeof(uint64_t), nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm->device, out.het_hom.data(), bufs.d_het_hom, total * sizeof(uint64_t), nullptr);
  }
  fmh_check(status);
  {
    py::gil_scoped_release nogil;
    status = fmh_kinship_stats(out.both.data(), out.het_het.data(), out.ibs0.data(), out.het_hom.data(), n, out.phi.data(), out.ibs_distance.data());
  }
  fmh_check(status);
  return out;
}

Kinship kinship(const py::object& variants, const py::object& samples, const py::object& sites, const py::object& region) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "kinship takes");
  vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  return kinship_over_rows(rows_in_play(store, region).resident(), std::move(list), sites);
}

Kinship population_kinship(const Population& pop, const py::object& sites) {
  diploid_only(pop, "kinship takes");
  return kinship_over_rows(rows_in_play(pop).resident(), population_samples(pop), sites);
}

void bind_kinship(py::module_& m) {
  py::class_<Kinship>(m, "Kinship")
      .def_property_readonly("samples", [](const Kinship& k) {
        py::array_t<int64_t> out((py::ssize_t)k.n());
        for (size_t i = 0; i < k.n(); ++i) out.mutable_data()[i] = k.samples[i];
        return out;
      })
      .def_property_readonly("sites", [](const Kinship& k) {
        py::array_t<int64_t> out((py::ssize_t)k.sites.size());
        if (!k.sites.empty()) memcpy(out.mutable_data(), k.sites.data(), k.sites.size() * sizeof(int64_t));
        return out;
      })
      .def_property_readonly("both", [](const Kinship& k) { return k.square(k.both); })
      .def_property_readonly("het_het", [](const Kinship& k) { return k.square(k.het_het); })
      .def_property_readonly("ibs0", [](const Kinship& k) { return k.square(k.ibs0); })
      .def_property_readonly("het_hom", [](const Kinship& k) { return k.square(k.het_hom); })
      .def_property_readonly("kinship", [](const Kinship& k) { return k.square(k.phi); })
      .def_property_readonly("ibs_distance", [](const Kinship& k) { return k.square(k.ibs_distance); })
      .def("unrelated", &Kinship::unrelated, py::arg("threshold"))
      .def("__repr__", &Kinship::repr);
  m.def("kinship", &kinship, py::arg("variants"), py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none());
}
