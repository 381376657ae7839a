// pymodule_qc.inc — ferromic.genotype_qc, Population.genotype_qc and the GenotypeQC result (included inside pymodule_stats.inc's namespace,
// after pymodule_rows.inc whose rows, sample and sites rules it uses).  An addition to the reference's surface: it has no genotype QC; the
// definition is include/ferromic_hip.h's (fmh_genotype_counts, fmh_hwe_exact, fmh_genotype_site_stats, fmh_genotype_site_weights,
// fmh_genotype_sample_stats).  Counts and the exact test's p come from the device; the other statistics are computed from the integers on
// the host by the library; the GIL is released around the C calls.

struct GenotypeQC {
  uint64_t n_samples = 0, kept_rows = 0;
  vector<uint32_t> samples;                      // sample numbers, ascending (empty when built from counts)
  vector<uint32_t> hom_ref, het, hom_alt;        // per site
  vector<double> call_rate, alt_frequency, maf, f_is, hwe_p;
  vector<uint64_t> s_hom_ref, s_het, s_hom_alt, s_weighted;  // per sample
  vector<double> s_call_rate, s_het_rate, s_f;
  bool has_hwe = false, has_f = false;

  // every statistic the host computes from the integers
  void estimate() {
    const size_t rows = hom_ref.size(), n = s_hom_ref.size();
    call_rate.assign(rows, 0.0); alt_frequency.assign(rows, 0.0); maf.assign(rows, 0.0); f_is.assign(rows, 0.0);
    s_call_rate.assign(n, 0.0); s_het_rate.assign(n, 0.0); s_f.assign(has_f ? n : 0, 0.0);
    const fmh_genotype_site_stats_out site{call_rate.data(), alt_frequency.data(), maf.data(), f_is.data(), nullptr};
    const fmh_genotype_sample_stats_out sample{s_call_rate.data(), s_het_rate.data(), has_f ? s_f.data() : nullptr};
    int status;
    {
      py::gil_scoped_release nogil;
      status = fmh_genotype_site_stats(hom_ref.data(), het.data(), hom_alt.data(), rows, n_samples, &site);
      if (status == FMH_OK)
        status = fmh_genotype_sample_stats(s_hom_ref.data(), s_het.data(), s_hom_alt.data(), has_f ? s_weighted.data() : nullptr, n, kept_rows, &sample);
    }
    fmh_check(status);
  }

  // a criterion that is not given is not tested; a NaN fails a criterion it is tested on (every comparison with a NaN is false)
  py::array_t<bool> site_filter(optional<double> min_call_rate, optional<double> min_maf, optional<double> min_hwe_p) const {
    if (min_hwe_p && !has_hwe) value_error("min_hwe_p needs the exact test: the result was computed with hwe=False");
    py::array_t<bool> out((py::ssize_t)hom_ref.size());
    bool* o = out.mutable_data();
    for (size_t i = 0; i < hom_ref.size(); ++i)
      o[i] = (!min_call_rate || call_rate[i] >= *min_call_rate) && (!min_maf || maf[i] >= *min_maf) && (!min_hwe_p || hwe_p[i] >= *min_hwe_p);
    return out;
  }
  py::array_t<bool> sample_filter(optional<double> min_call_rate, optional<double> max_abs_f) const {
    if (max_abs_f && !has_f) value_error("max_abs_f needs the inbreeding coefficient: the result was computed with inbreeding=False");
    py::array_t<bool> out((py::ssize_t)s_hom_ref.size());
    bool* o = out.mutable_data();
    for (size_t i = 0; i < s_hom_ref.size(); ++i)
      o[i] = (!min_call_rate || s_call_rate[i] >= *min_call_rate) && (!max_abs_f || std::fabs(s_f[i]) <= *max_abs_f);
    return out;
  }
  string repr() const { return "GenotypeQC(samples=" + std::to_string(s_hom_ref.size()) + ", sites=" + std::to_string(hom_ref.size()) + ")"; }
};

// A result from counts that were computed before (no device): the exact test runs on the host twin.
GenotypeQC genotype_qc_from_counts(const py::object& hom_ref, const py::object& het, const py::object& hom_alt, uint64_t n_samples,
                                   const py::object& sample_hom_ref, const py::object& sample_het, const py::object& sample_hom_alt, uint64_t kept_rows,
                                   const py::object& weighted_called) {
  GenotypeQC out;
  out.n_samples = n_samples;
  out.kept_rows = kept_rows;
  out.hom_ref = vector_arg<uint32_t>(hom_ref, "hom_ref", 0, false);
  out.het = vector_arg<uint32_t>(het, "het", out.hom_ref.size(), true);
  out.hom_alt = vector_arg<uint32_t>(hom_alt, "hom_alt", out.hom_ref.size(), true);
  out.s_hom_ref = vector_arg<uint64_t>(sample_hom_ref, "sample_hom_ref", 0, false);
  out.s_het = vector_arg<uint64_t>(sample_het, "sample_het", out.s_hom_ref.size(), true);
  out.s_hom_alt = vector_arg<uint64_t>(sample_hom_alt, "sample_hom_alt", out.s_hom_ref.size(), true);
  out.has_f = !weighted_called.is_none();
  if (out.has_f) out.s_weighted = vector_arg<uint64_t>(weighted_called, "weighted_called", out.s_hom_ref.size(), true);
  out.has_hwe = true;
  out.hwe_p.assign(out.hom_ref.size(), 0.0);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_hwe_exact_host(out.hom_ref.data(), out.het.data(), out.hom_alt.data(), out.hom_ref.size(), out.hwe_p.data());
  }
  fmh_check(status);
  out.estimate();
  return out;
}

GenotypeQC genotype_qc_over_rows(const ResidentRows& rows, vector<uint32_t> samples, const py::object& sites, bool hwe, bool inbreeding) {
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  GenotypeQC out;
  out.samples = std::move(samples);
  const size_t n = out.samples.size();
  if (n == 0) value_error("at least one sample is required for genotype QC");
  out.n_samples = n;
  out.has_hwe = hwe;
  out.has_f = inbreeding;
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  const uint8_t* keep_ptr = masked ? keep.data() : nullptr;
  out.s_hom_ref.assign(n, 0); out.s_het.assign(n, 0); out.s_hom_alt.assign(n, 0);
  if (inbreeding) out.s_weighted.assign(n, 0);
  if (dm && rc != 0) {
    out.hom_ref.assign(rc, 0); out.het.assign(rc, 0); out.hom_alt.assign(rc, 0);
    if (hwe) out.hwe_p.assign(rc, 0.0);
    DevBuf d_tracks(dm->device, 3 * rc * sizeof(uint32_t)), d_tables(dm->device, 4 * n * sizeof(uint64_t)), d_p(dm->device, hwe ? rc * sizeof(double) : 0);
    uint32_t* t = (uint32_t*)d_tracks.p;
    unsigned long long* s = (unsigned long long*)d_tables.p;
    const fmh_genotype_site_out site{t, t + rc, t + 2 * rc};
    const fmh_genotype_sample_out counted{s, s + n, s + 2 * n, nullptr}, weighted{nullptr, nullptr, nullptr, s + 3 * n};
    vector<uint32_t> weights(inbreeding ? rc : 0);
    int status;
    {
      py::gil_scoped_release nogil;
      const int dev = dm->device;
      status = fmh_device_zero(dev, d_tables.p, 4 * n * sizeof(uint64_t), nullptr);
      if (status == FMH_OK) status = fmh_genotype_counts(dm->h, out.samples.data(), n, r0, rc, keep_ptr, nullptr, &site, &counted, &out.kept_rows, nullptr);
      if (status == FMH_OK && hwe) status = fmh_hwe_exact(site.d_hom_ref, site.d_het, site.d_hom_alt, rc, (double*)d_p.p, dev, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, out.hom_ref.data(), site.d_hom_ref, rc * sizeof(uint32_t), nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, out.het.data(), site.d_het, rc * sizeof(uint32_t), nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, out.hom_alt.data(), site.d_hom_alt, rc * sizeof(uint32_t), nullptr);
      if (status == FMH_OK && hwe) status = fmh_copy_to_host(dev, out.hwe_p.data(), d_p.p, rc * sizeof(double), nullptr);
      // the second pass: the per-site expectation as fixed-point row weights, summed over each sample's own called sites
      if (status == FMH_OK && inbreeding) status = fmh_genotype_site_weights(out.hom_ref.data(), out.het.data(), out.hom_alt.data(), rc, weights.data());
      if (status == FMH_OK && inbreeding)
        status = fmh_genotype_counts(dm->h, out.samples.data(), n, r0, rc, keep_ptr, weights.data(), nullptr, &weighted, nullptr, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, out.s_hom_ref.data(), counted.d_hom_ref, n * sizeof(uint64_t), nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, out.s_het.data(), counted.d_het, n * sizeof(uint64_t), nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dev, out.s_hom_alt.data(), counted.d_hom_alt, n * sizeof(uint64_t), nullptr);
      if (status == FMH_OK && inbreeding) status = fmh_copy_to_host(dev, out.s_weighted.data(), weighted.d_weighted_called, n * sizeof(uint64_t), nullptr);
    }
    fmh_check(status);
  }
  out.estimate();
  return out;
}

GenotypeQC genotype_qc(const py::object& variants, const py::object& samples, const py::object& sites, const py::object& region, bool hwe,
                       bool inbreeding) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "genotype QC takes");
  vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  return genotype_qc_over_rows(rows_in_play(store, region).resident(), std::move(list), sites, hwe, inbreeding);
}

GenotypeQC population_genotype_qc(const Population& pop, const py::object& sites, bool hwe, bool inbreeding) {
  diploid_only(pop, "genotype QC takes");
  return genotype_qc_over_rows(rows_in_play(pop).resident(), population_samples(pop), sites, hwe, inbreeding);
}

void bind_qc(py::module_& m) {
  py::class_<GenotypeQC>(m, "GenotypeQC")
      .def_static("from_counts", &genotype_qc_from_counts, py::arg("hom_ref"), py::arg("het"), py::arg("hom_alt"), py::arg("n_samples"),
                  py::arg("sample_hom_ref"), py::arg("sample_het"), py::arg("sample_hom_alt"), py::arg("kept_rows"),
                  py::arg("weighted_called") = py::none())
      .def_property_readonly("samples", [](const GenotypeQC& q) {
        py::array_t<int64_t> out((py::ssize_t)q.samples.size());
        for (size_t i = 0; i < q.samples.size(); ++i) out.mutable_data()[i] = q.samples[i];
        return out;
      })
      .def_property_readonly("kept_rows", [](const GenotypeQC& q) { return q.kept_rows; })
      .def_property_readonly("hom_ref", [](const GenotypeQC& q) { return array_of(q.hom_ref); })
      .def_property_readonly("het", [](const GenotypeQC& q) { return array_of(q.het); })
      .def_property_readonly("hom_alt", [](const GenotypeQC& q) { return array_of(q.hom_alt); })
      .def_property_readonly("call_rate", [](const GenotypeQC& q) { return array_of(q.call_rate); })
      .def_property_readonly("alt_frequency", [](const GenotypeQC& q) { return array_of(q.alt_frequency); })
      .def_property_readonly("maf", [](const GenotypeQC& q) { return array_of(q.maf); })
      .def_property_readonly("f_is", [](const GenotypeQC& q) { return array_of(q.f_is); })
      .def_property_readonly("hwe_p", [](const GenotypeQC& q) -> py::object { return q.has_hwe ? py::object(array_of(q.hwe_p)) : py::object(py::none()); })
      .def_property_readonly("sample_hom_ref", [](const GenotypeQC& q) { return array_of(q.s_hom_ref); })
      .def_property_readonly("sample_het", [](const GenotypeQC& q) { return array_of(q.s_het); })
      .def_property_readonly("sample_hom_alt", [](const GenotypeQC& q) { return array_of(q.s_hom_alt); })
      .def_property_readonly("sample_weighted_called", [](const GenotypeQC& q) -> py::object { return q.has_f ? py::object(array_of(q.s_weighted)) : py::object(py::none()); })
      .def_property_readonly("sample_call_rate", [](const GenotypeQC& q) { return array_of(q.s_call_rate); })
      .def_property_readonly("sample_het_rate", [](const GenotypeQC& q) { return array_of(q.s_het_rate); })
      .def_property_readonly("sample_f", [](const GenotypeQC& q) -> py::object { return q.has_f ? py::object(array_of(q.s_f)) : py::object(py::none()); })
      .def("site_filter", &GenotypeQC::site_filter, py::arg("min_call_rate") = py::none(), py::arg("min_maf") = py::none(),
           py::arg("min_hwe_p") = py::none())
      .def("sample_filter", &GenotypeQC::sample_filter, py::arg("min_call_rate") = py::none(), py::arg("max_abs_f") = py::none())
      .def("__repr__", &GenotypeQC::repr);
  m.def("genotype_qc", &genotype_qc, py::arg("variants"), py::arg("samples") = py::none(), py::arg("sites") = py::none(),
        py::arg("region") = py::none(), py::arg("hwe") = true, py::arg("inbreeding") = true);
}
