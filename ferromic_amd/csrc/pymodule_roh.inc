// pymodule_roh.inc — ferromic.runs_of_homozygosity, Population.runs_of_homozygosity and the HomozygosityRuns result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample and sites rules it uses, and pymodule_segments.inc).  An addition to the reference's
// surface: it has no runs of homozygosity; the definition is include/ferromic_hip.h's (fmh_roh_scan, fmh_roh_need, fmh_roh_sort_segments).
// Every integer comes from the device; F_ROH and the coverage track are computed from them on the host; the GIL is released around the C
// calls.  Positions go to the library relative to the first row in play.

struct HomozygosityRuns : SegmentResult<fmh_roh_segment> {  // segments sorted by (sample, first_row)
  vector<uint64_t> n_runs, total_sites, total_length, longest;    // per sample
  vector<uint64_t> bin_runs, bin_length;                          // [n][n_bins]
  size_t n_bins = 0;

  size_t n() const { return n_runs.size(); }
  py::array_t<double> f_roh(const py::object& genome_length) const { return genome_fraction(total_length, genome_length, {(py::ssize_t)n()}); }
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
    d["window"] = params.window; d["window_het"] = params.window_het; d["window_missing"] = params.window_missing;
    d["window_threshold"] = threshold;
    py::list need;
    for (uint32_t c = 0; c <= params.window; ++c) need.append((int)params.need[c]);
    d["need"] = need;
    d["min_sites"] = params.min_sites; d["min_length"] = params.min_length;
    d["max_gap"] = none_or_u32(params.max_gap, 0); d["max_bp_per_site"] = none_or_u32(params.max_bp_per_site, 0);
    d["max_het"] = none_or_u32(params.max_het, 0xFFFFFFFFu); d["max_missing"] = none_or_u32(params.max_missing, 0xFFFFFFFFu);
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
  if (window < 1 || window > 64) value_error("window must be within 1 .. 64, got " + std::to_string(window));
  if (!(window_threshold >= 0.0 && window_threshold <= 1.0)) value_error("window_threshold must be within 0 .. 1");
  req.params.window = (uint32_t)window;
  req.params.window_het = u32_arg(window_het, "window_het");
  req.params.window_missing = u32_arg(window_missing, "window_missing");
  req.threshold = window_threshold;
  fmh_check_args(fmh_roh_need(window_threshold, (uint32_t)window, req.params.need));
  req.params.min_sites = u32_arg(min_sites, "min_sites");
  req.params.min_length = u32_arg(min_length, "min_length");
  req.params.max_gap = optional_u32_arg(max_gap, "max_gap", 0);
  req.params.max_bp_per_site = optional_u32_arg(max_bp_per_site, "max_bp_per_site", 0);
  req.params.max_het = optional_u32_arg(max_het, "max_het", 0xFFFFFFFFu);
  req.params.max_missing = optional_u32_arg(max_missing, "max_missing", 0xFFFFFFFFu);
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
  out.take_positions(positions);
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, out.positions.size(), &masked);
  const vector<uint32_t> edges = roh_bins_arg(length_bins);
  out.has_segments = true;
  out.segments.resize(count);
  for (size_t i = 0; i < count; ++i) {
    if (who[i] >= out.samples.size()) value_error("segment " + std::to_string(i) + " names entry " + std::to_string(who[i]) + " of " + std::to_string(out.samples.size()) + " samples");
    out.check_segment_rows(i, first[i], last[i]);
    out.segments[i] = fmh_roh_segment{who[i], n_sites[i], n_het[i], n_missing[i], first[i], last[i]};
  }
  fmh_check_args(fmh_roh_sort_segments(out.segments.data(), count));
  out.span(keep, masked);
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
  check_positions_in_play(out.positions, "runs of homozygosity need", "scan");
  const vector<uint32_t> device_x = device_positions(out.positions, dm->variants, r0);
  out.span(keep, masked);
  const size_t nb = out.n_bins, words = 4 * n + 2 * n * nb;
  DevBuf d_tables(dm->device, words * sizeof(uint64_t));
  unsigned long long* t = (unsigned long long*)d_tables.p;
  const fmh_roh_out tables{t, t + n, t + 2 * n, t + 3 * n, nb ? t + 4 * n : nullptr, nb ? t + 4 * n + n * nb : nullptr};
  vector<uint64_t> host(words);
  const uint8_t* keep_ptr = masked ? keep.data() : nullptr;
  scan_segments(dm->device, req.segments, n, d_tables, host, out.segments,
                [&](bool with_tables, fmh_roh_segment* d_segments, size_t capacity, uint64_t* count) {
                  return fmh_roh_scan(dm->h, out.samples.data(), n, r0, rc, keep_ptr, device_x.data(), &req.params, with_tables ? &tables : nullptr, d_segments,
                                      capacity, count, nullptr);
                },
                fmh_roh_sort_segments);
  out.n_runs.assign(host.begin(), host.begin() + n);
  out.total_sites.assign(host.begin() + n, host.begin() + 2 * n);
  out.total_length.assign(host.begin() + 2 * n, host.begin() + 3 * n);
  out.longest.assign(host.begin() + 3 * n, host.begin() + 4 * n);
  out.bin_runs.assign(host.begin() + 4 * n, host.begin() + 4 * n + n * nb);
  out.bin_length.assign(host.begin() + 4 * n + n * nb, host.end());
  return out;
}

void bind_roh(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<HomozygosityRuns> runs(m, "HomozygosityRuns");
  bind_segment_result(runs);
  runs.def_static("from_segments", &roh_from_segments, py::arg("samples"), py::arg("segment_sample"), py::arg("segment_first_row"),
                  py::arg("segment_last_row"), py::arg("segment_sites"), py::arg("segment_het"), py::arg("segment_missing"), py::arg("positions"),
                  py::arg("sites") = py::none(), py::arg("length_bins") = py::none())
      .def_property_readonly("n_runs", [](const HomozygosityRuns& r) { return array_of(r.n_runs); })
      .def_property_readonly("total_sites", [](const HomozygosityRuns& r) { return array_of(r.total_sites); })
      .def_property_readonly("total_length", [](const HomozygosityRuns& r) { return array_of(r.total_length); })
      .def_property_readonly("longest", [](const HomozygosityRuns& r) { return array_of(r.longest); })
      .def_property_readonly("bin_runs", [](const HomozygosityRuns& r) { return r.table(r.bin_runs, r.n_bins); })
      .def_property_readonly("bin_length", [](const HomozygosityRuns& r) { return r.table(r.bin_length, r.n_bins); })
      .def_property_readonly("segment_sample", [](const HomozygosityRuns& r) { return r.segment_column<uint32_t>([](const fmh_roh_segment& s) { return s.sample; }); })
      .def_property_readonly("segment_het", [](const HomozygosityRuns& r) { return r.segment_column<uint32_t>([](const fmh_roh_segment& s) { return s.n_het; }); })
      .def("f_roh", &HomozygosityRuns::f_roh, py::arg("genome_length") = py::none())
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
