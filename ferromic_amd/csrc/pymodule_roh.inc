// pymodule_roh.inc — ferromic.runs_of_homozygosity, Population.runs_of_homozygosity and the HomozygosityRuns result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample and sites rules it uses).  An addition to the reference's
// surface: it has no runs of homozygosity; the definition is include/ferromic_hip.h's (fmh_roh_scan, fmh_roh_need, fmh_roh_sort_segments).
// Every integer comes from the device; F_ROH and the coverage track are computed from them on the host; the GIL is released around the C
// calls.  Positions go to the library relative to the first row in play.

struct HomozygosityRuns {
  vector<uint32_t> samples;                                       // sample numbers, ascending
  vector<uint64_t> n_runs, total_sites, total_length, longest;    // per sample
  vector<uint64_t> bin_runs, bin_length;                          // [n][n_bins]
  size_t n_bins = 0;
  uint64_t kept_rows = 0;
  bool has_segments = false, has_span = false;
  vector<fmh_roh_segment> segments;                               // sorted by (sample, first_row); rows are rows in play
  vector<int64_t> positions;                                      // of the rows in play
  int64_t span_first = 0, span_last = 0;                          // positions of the first and last kept row (has_span)
  py::object params = py::none();

  size_t n() const { return n_runs.size(); }
  void need_segments() const { if (!has_segments) value_error("the result holds no segments: it was computed with segments=False"); }
  template <class T, class F> py::array_t<T> segment_column(F get) const {
    need_segments();
    py::array_t<T> out((py::ssize_t)segments.size());
    for (size_t i = 0; i < segments.size(); ++i) out.mutable_data()[i] = (T)get(segments[i]);
    return out;
  }
  py::array_t<uint64_t> bins(const vector<uint64_t>& v) const {
    py::array_t<uint64_t> out({(py::ssize_t)n(), (py::ssize_t)n_bins});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(uint64_t));
    return out;
  }
  py::array_t<double> f_roh(const py::object& genome_length) const {
    double length = std::numeric_limits<double>::quiet_NaN();
    if (!genome_length.is_none()) {
      length = genome_length.cast<double>();
      if (!(length > 0.0)) value_error("genome_length must be positive");
    } else if (has_span) length = (double)(span_last - span_first + 1);
    py::array_t<double> out((py::ssize_t)n());
    for (size_t i = 0; i < n(); ++i) out.mutable_data()[i] = (double)total_length[i] / length;
    return out;
  }
  // per row in play: the selected samples with a qualifying run over it (every row of [first_row, last_row]), by a difference array
  py::array_t<uint32_t> site_coverage() const {
    need_segments();
    const size_t rows = positions.size();
    vector<int64_t> diff(rows + 1, 0);
    for (const fmh_roh_segment& s : segments) {
      if (s.last_row >= rows || s.first_row > s.last_row) value_error("a segment lies outside the " + std::to_string(rows) + " rows in play");
      ++diff[s.first_row];
      --diff[s.last_row + 1];
    }
    py::array_t<uint32_t> out((py::ssize_t)rows);
    int64_t depth = 0;
    for (size_t r = 0; r < rows; ++r) { depth += diff[r]; out.mutable_data()[r] = (uint32_t)depth; }
    return out;
  }
  string repr() const {
    uint64_t runs = 0;
    for (uint64_t r : n_runs) runs += r;
    return "HomozygosityRuns(samples=" + std::to_string(n()) + ", kept_rows=" + std::to_string(kept_rows) + ", runs=" + std::to_string(runs) + ")";
  }
};

// the length bins: None (or no edge) = no bins, else up to seven strictly ascending edges below 2^32: len + 1 bins
vector<uint32_t> roh_bins_arg(const py::object& length_bins) {
  vector<uint32_t> edges;
  if (length_bins.is_none()) return edges;
  for (const py::handle& item : py::iter(length_bins)) {
    if (!is_intlike(item)) raise(PyExc_TypeError, "length_bins must be integers");
    const int64_t e = to_i64(item);
    if (e < 0 || e > (int64_t)0xFFFFFFFFll) value_error("a length bin edge must be within 0 .. 2^32 - 1");
    if (!edges.empty() && (int64_t)edges.back() >= e) value_error("length_bins must be strictly ascending");
    edges.push_back((uint32_t)e);
  }
  if (edges.size() > 7) value_error(std::to_string(edges.size()) + " length bin edges: at most 7 (8 bins) are taken");
  return edges;
}

// what the caller asked for, checked before anything is read or uploaded
struct RohRequest {
  fmh_roh_params params{};
  double threshold = 0.0;
  vector<uint32_t> edges;
  bool segments = true;
  py::dict as_dict() const {
    py::dict d;
    auto limit = [](uint32_t v) -> py::object { return v == 0xFFFFFFFFu ? py::object(py::none()) : py::object(py::int_(v)); };
    auto unless_zero = [](uint32_t v) -> py::object { return v == 0 ? py::object(py::none()) : py::object(py::int_(v)); };
    d["window"] = params.window; d["window_het"] = params.window_het; d["window_missing"] = params.window_missing;
    d["window_threshold"] = threshold;
    py::list need;
    for (uint32_t c = 0; c <= params.window; ++c) need.append((int)params.need[c]);
    d["need"] = need;
    d["min_sites"] = params.min_sites; d["min_length"] = params.min_length;
    d["max_gap"] = unless_zero(params.max_gap); d["max_bp_per_site"] = unless_zero(params.max_bp_per_site);
    d["max_het"] = limit(params.max_het); d["max_missing"] = limit(params.max_missing);
    py::list bins;
    for (uint32_t e : edges) bins.append(e);
    d["length_bins"] = edges.empty() ? py::object(py::none()) : py::object(bins);
    return d;
  }
};
RohRequest roh_parse_request(int64_t window, int64_t window_het, int64_t window_missing, double window_threshold, int64_t min_sites, int64_t min_length,
                             const py::object& max_gap, const py::object& max_bp_per_site, const py::object& max_het, const py::object& max_missing,
                             const py::object& length_bins, bool segments) {
  RohRequest req;
  auto u32_of = [](int64_t v, const char* name) -> uint32_t {
    if (v < 0 || v > (int64_t)0xFFFFFFFFll) value_error(string(name) + " must be within 0 .. 2^32 - 1");
    return (uint32_t)v;
  };
  auto optional_u32 = [&](const py::object& o, const char* name, uint32_t none) -> uint32_t {
    if (o.is_none()) return none;
    if (!is_intlike(o)) value_error(string(name) + " must be an integer or None");
    const int64_t v = to_i64(o);
    if (v < 0 || v >= (int64_t)0xFFFFFFFFll) value_error(string(name) + " must be within 0 .. 2^32 - 2 or None");
    return (uint32_t)v;
  };
  if (window < 1 || window > 64) value_error("window must be within 1 .. 64, got " + std::to_string(window));
  if (!(window_threshold >= 0.0 && window_threshold <= 1.0)) value_error("window_threshold must be within 0 .. 1");
  req.params.window = (uint32_t)window;
  req.params.window_het = u32_of(window_het, "window_het");
  req.params.window_missing = u32_of(window_missing, "window_missing");
  req.threshold = window_threshold;
  fmh_check_args(fmh_roh_need(window_threshold, (uint32_t)window, req.params.need));
  req.params.min_sites = u32_of(min_sites, "min_sites");
  req.params.min_length = u32_of(min_length, "min_length");
  req.params.max_gap = optional_u32(max_gap, "max_gap", 0);
  req.params.max_bp_per_site = optional_u32(max_bp_per_site, "max_bp_per_site", 0);
  req.params.max_het = optional_u32(max_het, "max_het", 0xFFFFFFFFu);
  req.params.max_missing = optional_u32(max_missing, "max_missing", 0xFFFFFFFFu);
  req.edges = roh_bins_arg(length_bins);
  req.params.n_bins = req.edges.empty() ? 0 : (uint32_t)req.edges.size() + 1;
  for (size_t b = 0; b < req.edges.size(); ++b) req.params.bin_edges[b] = req.edges[b];
  req.segments = segments;
  return req;
}

// the tables of a result from its segments (host): from_segments, and what a region without a row answers
void roh_summarise(HomozygosityRuns& out, const vector<uint32_t>& edges) {
  const size_t n = out.samples.size();
  out.n_bins = edges.empty() ? 0 : edges.size() + 1;
  out.n_runs.assign(n, 0); out.total_sites.assign(n, 0); out.total_length.assign(n, 0); out.longest.assign(n, 0);
  out.bin_runs.assign(n * out.n_bins, 0); out.bin_length.assign(n * out.n_bins, 0);
  for (const fmh_roh_segment& s : out.segments) {
    const uint64_t length = (uint64_t)(out.positions[s.last_row] - out.positions[s.first_row]) + 1;
    ++out.n_runs[s.sample];
    out.total_sites[s.sample] += s.n_sites;
    out.total_length[s.sample] += length;
    out.longest[s.sample] = std::max(out.longest[s.sample], length);
    if (out.n_bins) {
      size_t b = 0;
      for (uint32_t e : edges) b += e <= length ? 1 : 0;
      ++out.bin_runs[s.sample * out.n_bins + b];
      out.bin_length[s.sample * out.n_bins + b] += length;
    }
  }
}

// A result from segments that were computed before (no device): `segment_sample` holds positions in `samples`, rows are rows of `positions`.
HomozygosityRuns roh_from_segments(const py::object& samples, const py::object& segment_sample, const py::object& segment_first_row,
                                   const py::object& segment_last_row, const py::object& segment_sites, const py::object& segment_het,
                                   const py::object& segment_missing, const py::object& positions, const py::object& sites,
                                   const py::object& length_bins) {
  HomozygosityRuns out;
  out.samples = vector_arg<uint32_t>(samples, "samples", 0, false);
  const vector<uint32_t> who = vector_arg<uint32_t>(segment_sample, "segment_sample", 0, false);
  const size_t count = who.size();
  const vector<uint64_t> first = vector_arg<uint64_t>(segment_first_row, "segment_first_row", count, true);
  const vector<uint64_t> last = vector_arg<uint64_t>(segment_last_row, "segment_last_row", count, true);
  const vector<uint32_t> n_sites = vector_arg<uint32_t>(segment_sites, "segment_sites", count, true);
  const vector<uint32_t> n_het = vector_arg<uint32_t>(segment_het, "segment_het", count, true);
  const vector<uint32_t> n_missing = vector_arg<uint32_t>(segment_missing, "segment_missing", count, true);
  out.positions = vector_arg<int64_t>(positions, "positions", 0, false);
  const size_t rows = out.positions.size();
  for (size_t r = 1; r < rows; ++r)
    if (out.positions[r] < out.positions[r - 1]) value_error("the positions descend at row " + std::to_string(r));
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rows, &masked);
  const vector<uint32_t> edges = roh_bins_arg(length_bins);
  out.has_segments = true;
  out.segments.resize(count);
  for (size_t i = 0; i < count; ++i) {
    if (who[i] >= out.samples.size()) value_error("segment " + std::to_string(i) + " names entry " + std::to_string(who[i]) + " of " + std::to_string(out.samples.size()) + " samples");
    if (first[i] > last[i] || last[i] >= rows) value_error("segment " + std::to_string(i) + " lies outside the " + std::to_string(rows) + " rows");
    out.segments[i] = fmh_roh_segment{who[i], n_sites[i], n_het[i], n_missing[i], first[i], last[i]};
  }
  fmh_check_args(fmh_roh_sort_segments(out.segments.data(), count));
  for (size_t r = 0; r < rows; ++r) {
    if (masked && !keep[r]) continue;
    if (!out.has_span) { out.has_span = true; out.span_first = out.positions[r]; }
    out.span_last = out.positions[r];
    ++out.kept_rows;
  }
  roh_summarise(out, edges);
  return out;
}

HomozygosityRuns roh_over_rows(const RowsInPlay& in_play, vector<uint32_t> samples, const py::object& sites, const RohRequest& req, const char* no_sample) {
  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = dm ? std::min(rows.rc, in_play.count) : 0;
  HomozygosityRuns out;
  out.samples = std::move(samples);
  const size_t n = out.samples.size();
  if (n == 0) value_error(no_sample);
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  out.params = req.as_dict();
  out.has_segments = req.segments;
  out.positions.assign(in_play.positions().begin(), in_play.positions().begin() + (std::ptrdiff_t)rc);
  roh_summarise(out, req.edges);  // zero tables of the right shapes
  if (rc == 0) return out;
  // positions relative to the first row in play, checked before any device use
  const vector<int64_t>& pos = out.positions;
  for (size_t r = 1; r < rc; ++r)
    if (pos[r] < pos[r - 1]) value_error("the positions descend at variant " + std::to_string(r) + ": runs of homozygosity need them in order");
  if ((uint64_t)(pos[rc - 1] - pos[0]) > 0xFFFFFFFFull)
    value_error("the positions span " + std::to_string(pos[rc - 1] - pos[0]) + ", more than 2^32 - 1: scan one chromosome (or a region of it) at a time");
  vector<uint32_t> device_x(dm->variants, 0);  // [variants] of the matrix: only the rows of the range are read
  for (size_t r = 0; r < rc; ++r) device_x[r0 + r] = (uint32_t)(pos[r] - pos[0]);
  for (size_t r = 0; r < rc; ++r) {
    if (masked && !keep[r]) continue;
    if (!out.has_span) { out.has_span = true; out.span_first = pos[r]; }
    out.span_last = pos[r];
  }
  const size_t nb = out.n_bins, words = 4 * n + 2 * n * nb;
  DevBuf d_tables(dm->device, words * sizeof(uint64_t));
  unsigned long long* t = (unsigned long long*)d_tables.p;
  const fmh_roh_out tables{t, t + n, t + 2 * n, t + 3 * n, nb ? t + 4 * n : nullptr, nb ? t + 4 * n + n * nb : nullptr};
  vector<uint64_t> host(words);
  size_t capacity = req.segments ? 64 + 8 * n : 0;  // the first guess; a second call only when the runs outnumber it
  uint64_t count = 0;
  const int dev = dm->device;
  const uint8_t* keep_ptr = masked ? keep.data() : nullptr;
  std::unique_ptr<DevBuf> d_seg;
  if (req.segments) d_seg = std::make_unique<DevBuf>(dev, capacity * sizeof(fmh_roh_segment));
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_roh_scan(dm->h, out.samples.data(), n, r0, rc, keep_ptr, device_x.data(), &req.params, &tables, d_seg ? (fmh_roh_segment*)d_seg->p : nullptr,
                          capacity, req.segments ? &count : nullptr, nullptr);
  }
  fmh_check(status);
  if (count > capacity) {  // the guess was short: the segments again, into a buffer that holds them all
    capacity = (size_t)count;
    d_seg = std::make_unique<DevBuf>(dev, capacity * sizeof(fmh_roh_segment));
    py::gil_scoped_release nogil;
    status = fmh_roh_scan(dm->h, out.samples.data(), n, r0, rc, keep_ptr, device_x.data(), &req.params, nullptr, (fmh_roh_segment*)d_seg->p, capacity, &count, nullptr);
  }
  fmh_check(status);
  {
    py::gil_scoped_release nogil;
    status = fmh_copy_to_host(dev, host.data(), d_tables.p, words * sizeof(uint64_t), nullptr);
    if (status == FMH_OK && count != 0) {
      out.segments.resize((size_t)count);
      status = fmh_copy_to_host(dev, out.segments.data(), d_seg->p, (size_t)count * sizeof(fmh_roh_segment), nullptr);
      if (status == FMH_OK) status = fmh_roh_sort_segments(out.segments.data(), out.segments.size());
    }
  }
  fmh_check(status);
  out.kept_rows = masked ? (uint64_t)std::count_if(keep.begin(), keep.end(), [](uint8_t k) { return k != 0; }) : rc;
  out.n_runs.assign(host.begin(), host.begin() + n);
  out.total_sites.assign(host.begin() + n, host.begin() + 2 * n);
  out.total_length.assign(host.begin() + 2 * n, host.begin() + 3 * n);
  out.longest.assign(host.begin() + 3 * n, host.begin() + 4 * n);
  out.bin_runs.assign(host.begin() + 4 * n, host.begin() + 4 * n + n * nb);
  out.bin_length.assign(host.begin() + 4 * n + n * nb, host.end());
  return out;
}

void bind_roh(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<HomozygosityRuns>(m, "HomozygosityRuns")
      .def_static("from_segments", &roh_from_segments, py::arg("samples"), py::arg("segment_sample"), py::arg("segment_first_row"),
                  py::arg("segment_last_row"), py::arg("segment_sites"), py::arg("segment_het"), py::arg("segment_missing"), py::arg("positions"),
                  py::arg("sites") = py::none(), py::arg("length_bins") = py::none())
      .def_property_readonly("samples", [](const HomozygosityRuns& r) {
        py::array_t<int64_t> out((py::ssize_t)r.samples.size());
        for (size_t i = 0; i < r.samples.size(); ++i) out.mutable_data()[i] = r.samples[i];
        return out;
      })
      .def_property_readonly("n_runs", [](const HomozygosityRuns& r) { return array_of(r.n_runs); })
      .def_property_readonly("total_sites", [](const HomozygosityRuns& r) { return array_of(r.total_sites); })
      .def_property_readonly("total_length", [](const HomozygosityRuns& r) { return array_of(r.total_length); })
      .def_property_readonly("longest", [](const HomozygosityRuns& r) { return array_of(r.longest); })
      .def_property_readonly("bin_runs", [](const HomozygosityRuns& r) { return r.bins(r.bin_runs); })
      .def_property_readonly("bin_length", [](const HomozygosityRuns& r) { return r.bins(r.bin_length); })
      .def_property_readonly("kept_rows", [](const HomozygosityRuns& r) { return r.kept_rows; })
      .def_property_readonly("params", [](const HomozygosityRuns& r) { return r.params; })
      .def_property_readonly("segment_sample", [](const HomozygosityRuns& r) { return r.segment_column<uint32_t>([](const fmh_roh_segment& s) { return s.sample; }); })
      .def_property_readonly("segment_first_row", [](const HomozygosityRuns& r) { return r.segment_column<uint64_t>([](const fmh_roh_segment& s) { return s.first_row; }); })
      .def_property_readonly("segment_last_row", [](const HomozygosityRuns& r) { return r.segment_column<uint64_t>([](const fmh_roh_segment& s) { return s.last_row; }); })
      .def_property_readonly("segment_start", [](const HomozygosityRuns& r) { return r.segment_column<int64_t>([&r](const fmh_roh_segment& s) { return r.positions[s.first_row]; }); })
      .def_property_readonly("segment_end", [](const HomozygosityRuns& r) { return r.segment_column<int64_t>([&r](const fmh_roh_segment& s) { return r.positions[s.last_row]; }); })
      .def_property_readonly("segment_sites", [](const HomozygosityRuns& r) { return r.segment_column<uint32_t>([](const fmh_roh_segment& s) { return s.n_sites; }); })
      .def_property_readonly("segment_het", [](const HomozygosityRuns& r) { return r.segment_column<uint32_t>([](const fmh_roh_segment& s) { return s.n_het; }); })
      .def_property_readonly("segment_missing", [](const HomozygosityRuns& r) { return r.segment_column<uint32_t>([](const fmh_roh_segment& s) { return s.n_missing; }); })
      .def("f_roh", &HomozygosityRuns::f_roh, py::arg("genome_length") = py::none())
      .def("site_coverage", &HomozygosityRuns::site_coverage)
      .def("__len__", &HomozygosityRuns::n)
      .def("__repr__", &HomozygosityRuns::repr);

  m.def("runs_of_homozygosity",
        [](const py::object& variants, const py::object& samples, const py::object& sites, const py::object& region, int64_t window, int64_t window_het,
           int64_t window_missing, double window_threshold, int64_t min_sites, int64_t min_length, const py::object& max_gap,
           const py::object& max_bp_per_site, const py::object& max_het, const py::object& max_missing, const py::object& length_bins, bool segments) {
          const RohRequest req = roh_parse_request(window, window_het, window_missing, window_threshold, min_sites, min_length, max_gap, max_bp_per_site,
                                                   max_het, max_missing, length_bins, segments);
          auto store = store_from_python(variants);
          diploid_only(store->P, (size_t)store->S, "runs of homozygosity take");
          vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
          return roh_over_rows(rows_in_play(store, region), std::move(list), sites, req, "at least one sample is required for runs of homozygosity");
        },
        py::arg("variants"), py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none(), py::arg("window") = 50,
        py::arg("window_het") = 1, py::arg("window_missing") = 5, py::arg("window_threshold") = 0.05, py::arg("min_sites") = 100,
        py::arg("min_length") = 1000000, py::arg("max_gap") = 1000000, py::arg("max_bp_per_site") = 50000, py::arg("max_het") = py::none(),
        py::arg("max_missing") = py::none(), py::arg("length_bins") = py::none(), py::arg("segments") = true);
  population.def("runs_of_homozygosity",
                 [](const Population& pop, const py::object& sites, int64_t window, int64_t window_het, int64_t window_missing, double window_threshold,
                    int64_t min_sites, int64_t min_length, const py::object& max_gap, const py::object& max_bp_per_site, const py::object& max_het,
                    const py::object& max_missing, const py::object& length_bins, bool segments) {
                   const RohRequest req = roh_parse_request(window, window_het, window_missing, window_threshold, min_sites, min_length, max_gap,
                                                            max_bp_per_site, max_het, max_missing, length_bins, segments);
                   diploid_only(pop, "runs of homozygosity take");
                   return roh_over_rows(rows_in_play(pop), population_samples(pop), sites, req,
                                        "at least one sample with both haplotypes in the population is required for runs of homozygosity");
                 },
                 py::arg("sites") = py::none(), py::arg("window") = 50, py::arg("window_het") = 1, py::arg("window_missing") = 5,
                 py::arg("window_threshold") = 0.05, py::arg("min_sites") = 100, py::arg("min_length") = 1000000, py::arg("max_gap") = 1000000,
                 py::arg("max_bp_per_site") = 50000, py::arg("max_het") = py::none(), py::arg("max_missing") = py::none(),
                 py::arg("length_bins") = py::none(), py::arg("segments") = true);
}
