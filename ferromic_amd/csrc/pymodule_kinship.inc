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

Kinship kinship_over_rows(const shared_ptr<DevMatrix>& dm, size_t r0, size_t rc, vector<uint32_t> samples, const py::object& sites) {
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
  if (store->S != 0 && store->P != 2) value_error("kinship takes diploid genotypes (ploidy 2), got ploidy " + std::to_string(store->P));
  vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  shared_ptr<const Store> sub = store;
  bool empty = store->S == 0;
  if (!empty && !region.is_none()) {
    const Region reg = build_region(region);
    const vector<int64_t> rows = region_len(reg) > 0 ? region_rows(*store, reg.start, reg.end) : vector<int64_t>();
    if (rows.empty()) empty = true;
    else sub = store_subset(store, rows);
  }
  if (empty) return kinship_over_rows(nullptr, 0, 0, std::move(list), sites);
  auto [dm, r0, rc] = sub->device_rows();
  return kinship_over_rows(dm, r0, rc, std::move(list), sites);
}

// the samples BOTH of whose haplotypes belong to the population, ascending, over its resident matrix
Kinship population_kinship(const Population& pop, const py::object& sites) {
  const int64_t ploidy = pop.dense ? pop.dense->ploidy : pop.store->P;
  const size_t count = pop.dense ? (size_t)pop.dense->variants : (size_t)pop.store->S;
  if (count != 0 && ploidy != 2) value_error("kinship takes diploid genotypes (ploidy 2), got ploidy " + std::to_string(ploidy));
  const int64_t limit = pop.dense ? pop.dense->samples : pop.store->first_sample_count();
  vector<uint8_t> sides((size_t)std::max<int64_t>(limit, 0), 0);
  for (auto& h : pop.haplotypes)
    if (h.first >= 0 && h.first < limit) sides[(size_t)h.first] |= h.second == kLeft ? 1 : 2;
  vector<uint32_t> list;
  for (size_t s = 0; s < sides.size(); ++s)
    if (sides[s] == 3) list.push_back((uint32_t)s);
  if (count == 0) return kinship_over_rows(nullptr, 0, 0, std::move(list), sites);
  const ResidentRows rows = resident_rows_of(pop);
  return kinship_over_rows(rows.dm, rows.r0, rows.rc, std::move(list), sites);
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
