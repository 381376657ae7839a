// pymodule_ld.inc — ferromic.ld_r2 / ld_prune and Population.ld_r2 / ld_prune (included inside pymodule_stats.inc's namespace, after the
// statistics whose argument handling they share).  An addition to the reference's surface: it has no linkage-disequilibrium code; the
// definition is include/ferromic_hip.h's (fmh_ld_band, fmh_ld_prune).  Sites are the rows of one resident matrix, the columns the haplotypes
// asked for; every number comes from the device, the GIL is released around the calls.

void ld_validate(size_t n_haplotypes, int64_t sites_apart, const char* what, const double* threshold) {
  if (n_haplotypes < 2) value_error("at least two haplotypes are required for linkage disequilibrium");
  if (sites_apart <= 0) value_error(string(what) + " must be a positive integer");
  if (threshold && !(*threshold >= 0.0 && *threshold <= 1.0)) value_error("r2_threshold must lie in [0, 1]");  // NaN fails both comparisons
}

py::array_t<double> ld_r2_rows(const ResidentRows& rows, size_t band) {
  const size_t r0 = rows.r0, rc = rows.rc;
  py::array_t<double> out(std::vector<py::ssize_t>{(py::ssize_t)rc, (py::ssize_t)band});
  if (rc == 0) return out;
  const DevMatrix& dm = *rows.dm;
  const shared_ptr<Groups> gp = groups_for(dm, {rows.mask});
  DevBuf d_r2(dm.device, rc * band * sizeof(double));
  fmh_ld_band_out bufs;
  memset(&bufs, 0, sizeof bufs);
  bufs.r2 = (double*)d_r2.p;
  double* host = out.mutable_data();
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_ld_band(dm.h, gp->h, r0, rc, r0 + rc, band, 0.0, &bufs, nullptr, nullptr, nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm.device, host, d_r2.p, rc * band * sizeof(double), nullptr);
  }
  fmh_check(status);
  return out;
}

py::array_t<bool> ld_prune_rows(const ResidentRows& rows, size_t window, double threshold) {
  const size_t r0 = rows.r0, rc = rows.rc;
  py::array_t<bool> out((py::ssize_t)rc);
  if (rc == 0) return out;
  const DevMatrix& dm = *rows.dm;
  const shared_ptr<Groups> gp = groups_for(dm, {rows.mask});
  vector<uint8_t> keep(rc, 0);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_ld_prune(dm.h, gp->h, r0, rc, window, threshold, keep.data(), nullptr);
  }
  fmh_check(status);
  bool* o = out.mutable_data();
  for (size_t i = 0; i < rc; ++i) o[i] = keep[i] != 0;
  return out;
}

// the rows of `region` (every variant when None) of a variant list and the haplotypes' columns, membership from the FIRST variant's sample
// count as per_site_diversity; `region` is read after the variants, and only when there is one
ResidentRows ld_rows(const py::object& variants, const vector<Hap>& haps, const py::object& region) {
  auto store = store_from_python(variants);
  return rows_in_play(store, region).resident(store->mask_for(haps, store->first_sample_count()));
}

py::array_t<double> ld_r2(const py::object& variants, const py::object& haplotypes, int64_t max_sites_apart, const py::object& region) {
  const vector<Hap> haps = parse_haplotypes(haplotypes);
  ld_validate(haps.size(), max_sites_apart, "max_sites_apart", nullptr);
  return ld_r2_rows(ld_rows(variants, haps, region), (size_t)max_sites_apart);
}

py::array_t<bool> ld_prune(const py::object& variants, const py::object& haplotypes, int64_t window_sites, double r2_threshold, const py::object& region) {
  const vector<Hap> haps = parse_haplotypes(haplotypes);
  ld_validate(haps.size(), window_sites, "window_sites", &r2_threshold);
  return ld_prune_rows(ld_rows(variants, haps, region), (size_t)window_sites, r2_threshold);
}

py::array_t<double> population_ld_r2(const Population& pop, int64_t max_sites_apart) {
  ld_validate(pop.haplotypes.size(), max_sites_apart, "max_sites_apart", nullptr);
  return ld_r2_rows(resident_rows_of(pop), (size_t)max_sites_apart);
}

py::array_t<bool> population_ld_prune(const Population& pop, int64_t window_sites, double r2_threshold) {
  ld_validate(pop.haplotypes.size(), window_sites, "window_sites", &r2_threshold);
  return ld_prune_rows(resident_rows_of(pop), (size_t)window_sites, r2_threshold);
}

void bind_ld(py::module_& m) {
  m.def("ld_r2", &ld_r2, py::arg("variants"), py::arg("haplotypes"), py::arg("max_sites_apart"), py::arg("region") = py::none());
  m.def("ld_prune", &ld_prune, py::arg("variants"), py::arg("haplotypes"), py::arg("window_sites"), py::arg("r2_threshold"), py::arg("region") = py::none());
}
