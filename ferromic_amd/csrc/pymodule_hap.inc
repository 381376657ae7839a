// pymodule_hap.inc — ferromic.garud_h, Population.garud_h and the class HaplotypeWindows (included inside pymodule_stats.inc's namespace,
// after pymodule_sfs.inc whose window parsing and row mapping it shares).  An addition to the reference's surface: it has no haplotype
// homozygosity; the definition is include/ferromic_hip.h's (fmh_haplotype_windows, fmh_haplotype_stats).  The class sizes come from the
// device as integers, the GIL is released around the call; the five statistics are fmh_haplotype_stats on the host.

struct HaplotypeWindows {
  size_t n = 0;
  vector<uint64_t> ranges;          // [n_windows][2]: the rows of the variants (of the region, when one was given) each window covers
  vector<fmh_hap_window> records;   // [n_windows]
  vector<fmh_hap_stats_out> stats;  // [n_windows]
  bool has_first = false;
  vector<uint32_t> first;           // [n_windows][n] when has_first

  size_t n_windows() const { return records.size(); }
  py::array_t<uint64_t> windows_array() const {
    py::array_t<uint64_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_windows(), 2});
    if (!ranges.empty()) memcpy(out.mutable_data(), ranges.data(), ranges.size() * sizeof(uint64_t));
    return out;
  }
  py::array_t<uint64_t> sum_squares() const {
    py::array_t<uint64_t> out((py::ssize_t)n_windows());
    for (size_t w = 0; w < n_windows(); ++w) out.mutable_data()[w] = records[w].sum_sq;
    return out;
  }
  py::array_t<uint32_t> distinct() const {
    py::array_t<uint32_t> out((py::ssize_t)n_windows());
    for (size_t w = 0; w < n_windows(); ++w) out.mutable_data()[w] = records[w].distinct;
    return out;
  }
  py::array_t<uint32_t> top_counts() const {
    py::array_t<uint32_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_windows(), 3});
    for (size_t w = 0; w < n_windows(); ++w)
      for (int k = 0; k < 3; ++k) out.mutable_data()[w * 3 + k] = records[w].top[k];
    return out;
  }
  py::array_t<double> f64_stat(double fmh_hap_stats_out::*field) const {
    py::array_t<double> out((py::ssize_t)n_windows());
    for (size_t w = 0; w < n_windows(); ++w) out.mutable_data()[w] = stats[w].*field;
    return out;
  }
  py::object first_identical() const {
    if (!has_first) return py::none();
    py::array_t<uint32_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_windows(), (py::ssize_t)n});
    if (!first.empty()) memcpy(out.mutable_data(), first.data(), first.size() * sizeof(uint32_t));
    return std::move(out);
  }
  string repr() const {
    return "HaplotypeWindows(sample_size=" + std::to_string(n) + ", windows=" + std::to_string(n_windows()) + (has_first ? ", partition=True" : "") + ")";
  }
};

// what the caller asked for, checked before anything is read or uploaded
struct HapRequest {
  optional<vector<Region>> windows;  // positions
  optional<size_t> size, step;       // counts of variants
};
HapRequest hap_parse_request(const py::object& windows, const py::object& size, const py::object& step) {
  HapRequest req;
  req.windows = sfs_parse_windows(windows);
  auto count_of = [](const py::object& o, const char* name) -> size_t {
    if (!is_intlike(o)) value_error(string(name) + " must be a positive integer (a count of variants)");
    const int64_t v = to_i64(o);
    if (v <= 0) value_error(string(name) + " must be a positive integer (a count of variants)");
    return (size_t)v;
  };
  if (!size.is_none()) req.size = count_of(size, "size");
  if (!step.is_none()) req.step = count_of(step, "step");
  if (req.windows && (req.size || req.step)) value_error("windows and size / step are mutually exclusive");
  if (req.step && !req.size) value_error("step needs size");
  return req;
}

// the row ranges [n_windows][2] of the request over `count` rows with these positions
vector<uint64_t> hap_row_ranges(const HapRequest& req, const vector<int64_t>& positions, size_t count) {
  vector<uint64_t> ranges;
  if (req.windows) {
    ranges.assign(req.windows->size() * 2, 0);  // a window that holds no row is the empty range [0, 0)
    if (count == 0) return ranges;
    const SfsRuns runs = sfs_runs(positions, count, 0, *req.windows);
    vector<uint8_t> seen(req.windows->size(), 0);
    for (size_t r = 0; r < runs.window_of.size(); ++r) {
      const size_t w = runs.window_of[r];
      if (seen[w])
        value_error("window " + std::to_string(w) + " covers more than one run of rows (the positions do not ascend): identical-haplotype classes cannot be summed over runs");
      seen[w] = 1;
      ranges[2 * w] = runs.ranges[2 * r];
      ranges[2 * w + 1] = runs.ranges[2 * r + 1];
    }
    return ranges;
  }
  if (req.size) {
    const size_t size = *req.size, step = req.step ? *req.step : size;
    for (size_t begin = 0; begin + size <= count; begin += step) { ranges.push_back(begin); ranges.push_back(begin + size); }
    return ranges;
  }
  return {(uint64_t)0, (uint64_t)count};
}

size_t hap_sample_size(const vector<Hap>& haps, const vector<uint8_t>* mask) {
  if (haps.empty()) value_error("at least one haplotype is required for haplotype homozygosity");
  if (!mask) return 0;
  const size_t n = mask_count(*mask);
  if (n == 0) value_error("none of the haplotypes is a column of the variants");
  if (n > fmh_haplotype_max_members())
    value_error(std::to_string(n) + " haplotypes exceed the " + std::to_string(fmh_haplotype_max_members()) + " a haplotype window holds on chip");
  return n;
}

// the rows in play are made resident (the matrix uploaded) only when some window holds a row: an empty window is one class of everyone
HaplotypeWindows hap_over_rows(const HapColumns& cols, const HapRequest& req, const RowsInPlay& in_play, bool partition) {
  HaplotypeWindows out;
  const size_t n = cols.n;
  out.n = n;
  out.ranges = hap_row_ranges(req, in_play.positions(), in_play.count);
  out.has_first = partition;
  const size_t n_windows = out.ranges.size() / 2;
  fmh_hap_window everyone{};
  everyone.sum_sq = (uint64_t)n * n;
  everyone.distinct = 1;
  everyone.top[0] = (uint32_t)n;
  out.records.assign(n_windows, everyone);
  out.stats.resize(n_windows);
  if (partition) {
    if (n_windows > ((size_t)1 << 32) / n) value_error("a partition of " + std::to_string(n_windows) + " windows x " + std::to_string(n) + " haplotypes exceeds 2^32 entries");
    out.first.assign(n_windows * n, 0);
  }
  bool any_row = false;
  for (size_t w = 0; w < n_windows; ++w) any_row = any_row || out.ranges[2 * w + 1] > out.ranges[2 * w];
  if (any_row) {
    const ResidentRows rows = in_play.resident(cols.mask);
    vector<uint64_t> device_ranges = out.ranges;
    for (uint64_t& r : device_ranges) r += rows.r0;
    const DevMatrix& dm = *rows.dm;
    const shared_ptr<Groups> gp = groups_for(dm, {rows.mask});
    DevBuf d_out(dm.device, n_windows * sizeof(fmh_hap_window));
    std::unique_ptr<DevBuf> d_first;
    if (partition) d_first = std::make_unique<DevBuf>(dm.device, out.first.size() * sizeof(uint32_t));
    int status;
    {
      py::gil_scoped_release nogil;
      status = fmh_haplotype_windows(dm.h, gp->h, device_ranges.data(), n_windows, (fmh_hap_window*)d_out.p, d_first ? (uint32_t*)d_first->p : nullptr, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dm.device, out.records.data(), d_out.p, n_windows * sizeof(fmh_hap_window), nullptr);
      if (status == FMH_OK && partition) status = fmh_copy_to_host(dm.device, out.first.data(), d_first->p, out.first.size() * sizeof(uint32_t), nullptr);
    }
    fmh_check(status);
  }
  if (n_windows) fmh_check(fmh_haplotype_stats(out.records.data(), n_windows, n, out.stats.data()));
  return out;
}

HaplotypeWindows garud_h(const py::object& variants, const py::object& haplotypes, const py::object& region, const py::object& windows,
                         const py::object& size, const py::object& step, bool partition) {
  const vector<Hap> haps = parse_haplotypes(haplotypes);
  hap_sample_size(haps, nullptr);
  const HapRequest req = hap_parse_request(windows, size, step);
  const optional<Region> reg = region_arg(region);
  auto store = store_from_python(variants);
  const HapColumns cols = hap_columns(*store, haps, hap_sample_size);
  return hap_over_rows(cols, req, rows_in_play(store, reg), partition);
}

HaplotypeWindows population_garud_h(const Population& pop, const py::object& windows, const py::object& size, const py::object& step, bool partition) {
  hap_sample_size(pop.haplotypes, nullptr);
  const HapRequest req = hap_parse_request(windows, size, step);
  return hap_over_rows(hap_columns(pop, hap_sample_size), req, rows_in_play(pop), partition);
}

void bind_hap(py::module_& m) {
  py::class_<HaplotypeWindows>(m, "HaplotypeWindows")
      .def_property_readonly("sample_size", [](const HaplotypeWindows& h) { return h.n; })
      .def_property_readonly("windows", &HaplotypeWindows::windows_array)
      .def_property_readonly("sum_squares", &HaplotypeWindows::sum_squares)
      .def_property_readonly("distinct", &HaplotypeWindows::distinct)
      .def_property_readonly("top_counts", &HaplotypeWindows::top_counts)
      .def_property_readonly("h1", [](const HaplotypeWindows& h) { return h.f64_stat(&fmh_hap_stats_out::h1); })
      .def_property_readonly("h12", [](const HaplotypeWindows& h) { return h.f64_stat(&fmh_hap_stats_out::h12); })
      .def_property_readonly("h123", [](const HaplotypeWindows& h) { return h.f64_stat(&fmh_hap_stats_out::h123); })
      .def_property_readonly("h2_h1", [](const HaplotypeWindows& h) { return h.f64_stat(&fmh_hap_stats_out::h2_h1); })
      .def_property_readonly("haplotype_diversity", [](const HaplotypeWindows& h) { return h.f64_stat(&fmh_hap_stats_out::haplotype_diversity); })
      .def_property_readonly("first_identical", &HaplotypeWindows::first_identical)
      .def("__len__", &HaplotypeWindows::n_windows)
      .def("__repr__", &HaplotypeWindows::repr);
  m.def("garud_h", &garud_h, py::arg("variants"), py::arg("haplotypes"), py::arg("region") = py::none(), py::arg("windows") = py::none(),
        py::arg("size") = py::none(), py::arg("step") = py::none(), py::arg("partition") = false);
}
