// pymodule_sfs.inc — ferromic.site_frequency_spectrum / joint_site_frequency_spectrum, Population.site_frequency_spectrum and the classes
// SiteFrequencySpectrum / JointSiteFrequencySpectrum (included inside pymodule_stats.inc's namespace, after the row
// handling the statistics share).  An addition to the reference's surface: it has no site frequency spectrum; the definition is
// include/ferromic_hip.h's (fmh_sfs, fmh_sfs_joint, fmh_sfs_stats).  Counts come from the device, the GIL is released around the calls;
// the statistics are fmh_sfs_stats on the host, so they work on any spectrum (from_counts) without a device.

struct SiteFrequencySpectrum {
  size_t n = 0;
  bool windowed = false;          // counts is [n_windows][n + 1] rather than [n + 1]
  size_t n_windows = 1;
  vector<uint64_t> counts;        // [n_windows][n + 1]
  vector<uint64_t> multiallelic, incomplete;  // [n_windows]

  template <class T> py::array_t<T> shaped(const vector<T>& flat, size_t width) const {
    py::array_t<T> out = windowed ? py::array_t<T>(std::vector<py::ssize_t>{(py::ssize_t)n_windows, (py::ssize_t)width})
                                  : py::array_t<T>((py::ssize_t)width);
    if (!flat.empty()) memcpy(out.mutable_data(), flat.data(), flat.size() * sizeof(T));
    return out;
  }
  py::array_t<uint64_t> counts_array() const { return shaped(counts, n + 1); }
  py::object tally(const vector<uint64_t>& t) const {
    if (!windowed) return py::int_(t[0]);
    py::array_t<uint64_t> out((py::ssize_t)n_windows);
    if (n_windows) memcpy(out.mutable_data(), t.data(), n_windows * sizeof(uint64_t));
    return std::move(out);
  }
  py::array_t<uint64_t> folded() const {
    const size_t width = n / 2 + 1;
    vector<uint64_t> f(n_windows * width, 0);
    for (size_t w = 0; w < n_windows; ++w)
      for (size_t j = 0; j < width; ++j) {
        const uint64_t* row = counts.data() + w * (n + 1);
        f[w * width + j] = j == n - j ? row[j] : row[j] + row[n - j];
      }
    return shaped(f, width);
  }
  fmh_sfs_stats_out stats_of(size_t w) const {
    fmh_sfs_stats_out o;
    fmh_check(fmh_sfs_stats(counts.data() + w * (n + 1), n, &o));
    return o;
  }
  py::object f64_stat(double fmh_sfs_stats_out::*field) const {
    if (!windowed) return py::float_(stats_of(0).*field);
    py::array_t<double> out((py::ssize_t)n_windows);
    for (size_t w = 0; w < n_windows; ++w) out.mutable_data()[w] = stats_of(w).*field;
    return std::move(out);
  }
  py::object segregating() const {
    if (!windowed) return py::int_(stats_of(0).segregating_sites);
    py::array_t<uint64_t> out((py::ssize_t)n_windows);
    for (size_t w = 0; w < n_windows; ++w) out.mutable_data()[w] = stats_of(w).segregating_sites;
    return std::move(out);
  }
  string repr() const {
    return "SiteFrequencySpectrum(sample_size=" + std::to_string(n) + (windowed ? ", windows=" + std::to_string(n_windows) : string()) + ")";
  }
};

struct JointSiteFrequencySpectrum {
  size_t n0 = 0, n1 = 0;
  vector<uint64_t> counts;  // [n0 + 1][n1 + 1]
  uint64_t multiallelic = 0, incomplete = 0;
  py::array_t<uint64_t> counts_array() const {
    py::array_t<uint64_t> out(std::vector<py::ssize_t>{(py::ssize_t)(n0 + 1), (py::ssize_t)(n1 + 1)});
    memcpy(out.mutable_data(), counts.data(), counts.size() * sizeof(uint64_t));
    return out;
  }
  // the 1-D spectrum of population `axis` over the rows the joint spectrum binned
  py::array_t<uint64_t> marginal(int axis) const {
    if (axis != 0 && axis != 1) value_error("axis must be 0 or 1");
    const size_t width = axis == 0 ? n0 + 1 : n1 + 1;
    py::array_t<uint64_t> out((py::ssize_t)width);
    uint64_t* o = out.mutable_data();
    std::fill(o, o + width, (uint64_t)0);
    for (size_t a = 0; a <= n0; ++a)
      for (size_t b = 0; b <= n1; ++b) o[axis == 0 ? a : b] += counts[a * (n1 + 1) + b];
    return out;
  }
  string repr() const { return "JointSiteFrequencySpectrum(sample_sizes=(" + std::to_string(n0) + ", " + std::to_string(n1) + "))"; }
};

SiteFrequencySpectrum sfs_from_counts(const py::object& obj) {
  auto arr = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(obj);
  if (!arr || (arr.ndim() != 1 && arr.ndim() != 2)) value_error("counts must be a 1-D or 2-D array of non-negative integers");
  const size_t width = (size_t)arr.shape(arr.ndim() - 1);
  if (width < 2) value_error("a site frequency spectrum has at least two bins (sample size 1)");
  SiteFrequencySpectrum out;
  out.n = width - 1;
  out.windowed = arr.ndim() == 2;
  out.n_windows = out.windowed ? (size_t)arr.shape(0) : 1;
  out.counts.assign(arr.data(), arr.data() + out.n_windows * width);
  out.multiallelic.assign(out.n_windows, 0);
  out.incomplete.assign(out.n_windows, 0);
  return out;
}

// `windows`: None, or an iterable of (start, end) in the coordinates of `region`; raised before any device use
optional<vector<Region>> sfs_parse_windows(const py::object& windows) {
  if (windows.is_none()) return std::nullopt;
  vector<Region> out;
  for (py::handle w : windows) {
    if (!(py::isinstance<py::tuple>(w) || py::isinstance<py::list>(w)) || py::len(w) != 2) value_error("windows must be a sequence of (start, end) pairs");
    py::sequence s = py::reinterpret_borrow<py::sequence>(w);
    if (!is_intlike(s[0]) || !is_intlike(s[1])) value_error("windows must be a sequence of (start, end) pairs of integers");
    const int64_t start = to_i64(s[0]), end = to_i64(s[1]);
    if (end < start) value_error("window end must be greater than or equal to window start");
    out.push_back({start, end});
  }
  return out;
}

// The rows of `positions` (the rows [r0, r0 + positions.size()) of a resident matrix) inside every window, as runs of consecutive rows:
// one run per window when the positions ascend, whatever it takes otherwise.
struct SfsRuns {
  vector<uint64_t> ranges;   // [n_runs][2]
  vector<size_t> window_of;  // [n_runs]
};
SfsRuns sfs_runs(const vector<int64_t>& positions, size_t count, size_t r0, const vector<Region>& windows) {
  SfsRuns out;
  const bool ascending = std::is_sorted(positions.begin(), positions.begin() + (std::ptrdiff_t)count);
  for (size_t w = 0; w < windows.size(); ++w) {
    if (region_len(windows[w]) <= 0) continue;
    if (ascending) {
      const size_t lo = (size_t)(std::lower_bound(positions.begin(), positions.begin() + (std::ptrdiff_t)count, windows[w].start) - positions.begin());
      const size_t hi = (size_t)(std::upper_bound(positions.begin(), positions.begin() + (std::ptrdiff_t)count, windows[w].end) - positions.begin());
      if (hi > lo) { out.ranges.push_back(r0 + lo); out.ranges.push_back(r0 + hi); out.window_of.push_back(w); }
      continue;
    }
    for (size_t i = 0; i < count;) {
      auto inside = [&](size_t k) { return positions[k] >= windows[w].start && positions[k] <= windows[w].end; };
      if (!inside(i)) { ++i; continue; }
      size_t j = i + 1;
      while (j < count && inside(j)) ++j;
      out.ranges.push_back(r0 + i); out.ranges.push_back(r0 + j); out.window_of.push_back(w);
      i = j;
    }
  }
  return out;
}

// the spectra of a group of haplotypes over the windows (None: every row) of the rows in play, which are made resident (the matrix
// uploaded) only when some window holds a row
SiteFrequencySpectrum sfs_over_rows(const HapColumns& cols, const RowsInPlay& in_play, const optional<vector<Region>>& windows) {
  SiteFrequencySpectrum out;
  const size_t n = cols.n, count = in_play.count;
  out.n = n;
  out.windowed = windows.has_value();
  out.n_windows = windows ? windows->size() : 1;
  const size_t width = n + 1;
  out.counts.assign(out.n_windows * width, 0);
  out.multiallelic.assign(out.n_windows, 0);
  out.incomplete.assign(out.n_windows, 0);
  if (count == 0) return out;
  SfsRuns runs;
  if (windows) runs = sfs_runs(in_play.positions(), count, 0, *windows);
  else { runs.ranges = {(uint64_t)0, (uint64_t)count}; runs.window_of = {0}; }
  const size_t n_runs = runs.window_of.size();
  if (n_runs == 0) return out;
  const ResidentRows rows = in_play.resident(cols.mask);
  for (uint64_t& r : runs.ranges) r += rows.r0;
  const DevMatrix& dm = *rows.dm;
  const shared_ptr<Groups> gp = groups_for(dm, {rows.mask});
  DevBuf d_sfs(dm.device, n_runs * width * sizeof(uint64_t));
  vector<uint64_t> table(n_runs * width);
  vector<fmh_sfs_skipped> skipped(n_runs);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_sfs(dm.h, gp->h, runs.ranges.data(), n_runs, (uint64_t*)d_sfs.p, skipped.data(), nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm.device, table.data(), d_sfs.p, table.size() * sizeof(uint64_t), nullptr);
  }
  fmh_check(status);
  for (size_t r = 0; r < n_runs; ++r) {
    const size_t w = runs.window_of[r];
    for (size_t k = 0; k < width; ++k) out.counts[w * width + k] += table[r * width + k];
    out.multiallelic[w] += skipped[r].multiallelic;
    out.incomplete[w] += skipped[r].incomplete;
  }
  return out;
}

size_t sfs_sample_size(const vector<Hap>& haps, const vector<uint8_t>* mask) {
  if (haps.empty()) value_error("at least one haplotype is required for a site frequency spectrum");
  if (!mask) return 0;
  const size_t n = mask_count(*mask);
  if (n == 0) value_error("none of the haplotypes is a column of the variants");
  return n;
}

SiteFrequencySpectrum site_frequency_spectrum(const py::object& variants, const py::object& haplotypes, const py::object& region, const py::object& windows) {
  const vector<Hap> haps = parse_haplotypes(haplotypes);
  sfs_sample_size(haps, nullptr);
  const optional<vector<Region>> wins = sfs_parse_windows(windows);
  const optional<Region> reg = region_arg(region);
  auto store = store_from_python(variants);
  const HapColumns cols = hap_columns(*store, haps, sfs_sample_size);
  return sfs_over_rows(cols, rows_in_play(store, reg), wins);
}

SiteFrequencySpectrum population_sfs(const Population& pop, const py::object& windows) {
  sfs_sample_size(pop.haplotypes, nullptr);
  const optional<vector<Region>> wins = sfs_parse_windows(windows);
  return sfs_over_rows(hap_columns(pop, sfs_sample_size), rows_in_play(pop), wins);
}

JointSiteFrequencySpectrum joint_site_frequency_spectrum(const py::object& a, const py::object& b) {
  auto p1 = coerce_population(a), p2 = coerce_population(b);
  if (!variants_compatible(*p1->store, *p2->store)) vcf_error("Parse", "Variant slices differ in positions/length.");
  const bool same_dense = p1->dense && p1->dense == p2->dense;
  const bool same_store = !p1->dense && !p2->dense && p1->store == p2->store;
  if (!same_dense && !same_store)
    value_error("the joint site frequency spectrum needs two populations over ONE resident matrix: make both with with_haplotypes from one Population");
  JointSiteFrequencySpectrum out;
  sfs_sample_size(p1->haplotypes, nullptr);
  const HapColumns c1 = hap_columns(*p1, sfs_sample_size);
  sfs_sample_size(p2->haplotypes, nullptr);
  const HapColumns c2 = hap_columns(*p2, sfs_sample_size);
  out.n0 = c1.n;
  out.n1 = c2.n;
  out.counts.assign((out.n0 + 1) * (out.n1 + 1), 0);
  if (variant_count(*p1) == 0) return out;
  const ResidentRows r1 = resident_rows_of(*p1);
  const DevMatrix& dm = *r1.dm;
  const shared_ptr<Groups> gp = groups_for(dm, {r1.mask, c2.mask});
  DevBuf d_sfs(dm.device, out.counts.size() * sizeof(uint64_t));
  fmh_sfs_skipped skipped{0, 0};
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_sfs_joint(dm.h, gp->h, r1.r0, r1.rc, (uint64_t*)d_sfs.p, &skipped, nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm.device, out.counts.data(), d_sfs.p, out.counts.size() * sizeof(uint64_t), nullptr);
  }
  fmh_check(status);
  out.multiallelic = skipped.multiallelic;
  out.incomplete = skipped.incomplete;
  return out;
}

void bind_sfs(py::module_& m) {
  py::class_<SiteFrequencySpectrum>(m, "SiteFrequencySpectrum")
      .def_static("from_counts", &sfs_from_counts, py::arg("counts"))
      .def_property_readonly("counts", &SiteFrequencySpectrum::counts_array)
      .def_property_readonly("sample_size", [](const SiteFrequencySpectrum& s) { return s.n; })
      .def_property_readonly("multiallelic_sites", [](const SiteFrequencySpectrum& s) { return s.tally(s.multiallelic); })
      .def_property_readonly("incomplete_sites", [](const SiteFrequencySpectrum& s) { return s.tally(s.incomplete); })
      .def("folded", &SiteFrequencySpectrum::folded)
      .def_property_readonly("segregating_sites", &SiteFrequencySpectrum::segregating)
      .def_property_readonly("theta_pi", [](const SiteFrequencySpectrum& s) { return s.f64_stat(&fmh_sfs_stats_out::pi_sum); })
      .def_property_readonly("theta_w", [](const SiteFrequencySpectrum& s) { return s.f64_stat(&fmh_sfs_stats_out::theta_w_sum); })
      .def_property_readonly("theta_h", [](const SiteFrequencySpectrum& s) { return s.f64_stat(&fmh_sfs_stats_out::theta_h_sum); })
      .def_property_readonly("tajimas_d", [](const SiteFrequencySpectrum& s) { return s.f64_stat(&fmh_sfs_stats_out::tajima_d); })
      .def_property_readonly("fay_wu_h", [](const SiteFrequencySpectrum& s) { return s.f64_stat(&fmh_sfs_stats_out::fay_wu_h); })
      .def("__repr__", &SiteFrequencySpectrum::repr);
  py::class_<JointSiteFrequencySpectrum>(m, "JointSiteFrequencySpectrum")
      .def_property_readonly("counts", &JointSiteFrequencySpectrum::counts_array)
      .def_property_readonly("sample_sizes", [](const JointSiteFrequencySpectrum& s) { return py::make_tuple(s.n0, s.n1); })
      .def_property_readonly("multiallelic_sites", [](const JointSiteFrequencySpectrum& s) { return s.multiallelic; })
      .def_property_readonly("incomplete_sites", [](const JointSiteFrequencySpectrum& s) { return s.incomplete; })
      .def("marginal", &JointSiteFrequencySpectrum::marginal, py::arg("axis"))
      .def("__repr__", &JointSiteFrequencySpectrum::repr);
  m.def("site_frequency_spectrum", &site_frequency_spectrum, py::arg("variants"), py::arg("haplotypes"), py::arg("region") = py::none(),
        py::arg("windows") = py::none());
  m.def("joint_site_frequency_spectrum", &joint_site_frequency_spectrum, py::arg("population1"), py::arg("population2"));
}
