// pymodule_ibd.inc — ferromic.ibd_segments, Population.ibd_segments and the IbdSegments result (included inside pymodule_stats.inc's
// namespace, after pymodule_rows.inc whose rows, sample and sites rules it uses, and pymodule_segments.inc).  An addition to the reference's surface: it has no IBD
// segments; the definition is include/ferromic_hip.h's (fmh_ibd_scan, fmh_ibd_sort_segments).  Every integer comes from the device; the IBD
// fraction and the coverage track are computed from them on the host; the GIL is released around the C calls.  Positions go to the library
// relative to the first row in play.  A request with one sample or without a kept row is answered without a device.

struct IbdSegments : SegmentResult<fmh_ibd_segment> {  // segments sorted by (a, b, first_row)
  vector<uint64_t> n_segments, total_sites, total_length, longest;  // [n][n]
  uint32_t mode = FMH_IBD1;

  size_t n() const { return samples.size(); }
  py::array_t<double> ibd_fraction(const py::object& genome_length) const {
    return genome_fraction(total_length, genome_length, {(py::ssize_t)n(), (py::ssize_t)n()});
  }
  string repr() const {
    uint64_t total = 0;
    for (size_t i = 0; i < n(); ++i)
      for (size_t j = i + 1; j < n(); ++j) total += n_segments[i * n() + j];
    return string("IbdSegments(mode=") + (mode == FMH_IBD2 ? "ibd2" : "ibd1") + ", samples=" + std::to_string(n()) + ", kept_rows=" + std::to_string(kept_rows) +
           ", segments=" + std::to_string(total) + ")";
  }
};

uint32_t ibd_mode_arg(const string& mode) {
  if (mode == "ibd1") return FMH_IBD1;
  if (mode == "ibd2") return FMH_IBD2;
  value_error("mode must be \"ibd1\" or \"ibd2\", got \"" + mode + "\"");
  return 0;
}

// what the caller asked for, checked before anything is read or uploaded
struct IbdRequest {
  fmh_ibd_params params{};
  bool segments = true;
  py::dict as_dict() const {
    py::dict d;
    d["mode"] = params.mode == FMH_IBD2 ? "ibd2" : "ibd1";
    d["min_sites"] = params.min_sites; d["min_length"] = params.min_length;
    d["max_gap"] = none_or_u32(params.max_gap, 0); d["max_bp_per_site"] = none_or_u32(params.max_bp_per_site, 0);
    d["max_missing"] = none_or_u32(params.max_missing, 0xFFFFFFFFu);
    return d;
  }
};
IbdRequest ibd_parse_request(const string& mode, int64_t min_sites, int64_t min_length, const py::object& max_gap, const py::object& max_bp_per_site,
                             const py::object& max_missing, bool segments) {
  IbdRequest req;
  req.params.mode = ibd_mode_arg(mode);
  req.params.min_sites = u32_arg(min_sites, "min_sites");
  req.params.min_length = u32_arg(min_length, "min_length");
  req.params.max_gap = optional_u32_arg(max_gap, "max_gap", 0);
  req.params.max_bp_per_site = optional_u32_arg(max_bp_per_site, "max_bp_per_site", 0);
  req.params.max_missing = optional_u32_arg(max_missing, "max_missing", 0xFFFFFFFFu);
  req.segments = segments;
  return req;
}

// the tables of a result from its segments (host): from_segments, and what a request without a pair or a kept row answers
void ibd_summarise(IbdSegments& out) {
  const size_t n = out.samples.size();
  out.n_segments.assign(n * n, 0); out.total_sites.assign(n * n, 0); out.total_length.assign(n * n, 0); out.longest.assign(n * n, 0);
  for (const fmh_ibd_segment& s : out.segments) {
    const uint64_t length = (uint64_t)(out.positions[s.last_row] - out.positions[s.first_row]) + 1;
    for (size_t at : {(size_t)s.a * n + s.b, (size_t)s.b * n + s.a}) {
      ++out.n_segments[at];
      out.total_sites[at] += s.n_sites;
      out.total_length[at] += length;
      out.longest[at] = std::max(out.longest[at], length);
    }
  }
}

// A result from segments that were computed before (no device): `segment_a` < `segment_b` hold positions in `samples`, rows are rows of `positions`.
IbdSegments ibd_from_segments(const py::object& samples, const py::object& segment_a, const py::object& segment_b, const py::object& segment_first_row,
                              const py::object& segment_last_row, const py::object& segment_sites, const py::object& segment_missing,
                              const py::object& positions, const py::object& sites, const string& mode) {
  IbdSegments out;
  out.mode = ibd_mode_arg(mode);
  out.samples = vector_arg<uint32_t>(samples, "samples", 0, false);
  const vector<uint32_t> a = vector_arg<uint32_t>(segment_a, "segment_a", 0, false);
  const size_t count = a.size();
  const vector<uint32_t> b = vector_arg<uint32_t>(segment_b, "segment_b", count, true);
  const vector<uint64_t> first = vector_arg<uint64_t>(segment_first_row, "segment_first_row", count, true);
  const vector<uint64_t> last = vector_arg<uint64_t>(segment_last_row, "segment_last_row", count, true);
  const vector<uint32_t> n_sites = vector_arg<uint32_t>(segment_sites, "segment_sites", count, true);
  const vector<uint32_t> n_missing = vector_arg<uint32_t>(segment_missing, "segment_missing", count, true);
  out.take_positions(positions);
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, out.positions.size(), &masked);
  out.has_segments = true;
  out.segments.resize(count);
  for (size_t i = 0; i < count; ++i) {
    if (a[i] >= b[i] || b[i] >= out.samples.size())
      value_error("segment " + std::to_string(i) + " names the pair (" + std::to_string(a[i]) + ", " + std::to_string(b[i]) + ") of " + std::to_string(out.samples.size()) + " samples: a < b < n is required");
    out.check_segment_rows(i, first[i], last[i]);
    out.segments[i] = fmh_ibd_segment{a[i], b[i], n_sites[i], n_missing[i], first[i], last[i]};
  }
  fmh_check_args(fmh_ibd_sort_segments(out.segments.data(), count));
  out.span(keep, masked);
  ibd_summarise(out);
  return out;
}

IbdSegments ibd_over_rows(const RowsInPlay& in_play, vector<uint32_t> samples, const py::object& sites, const IbdRequest& req, const char* no_sample) {
  IbdSegments out;
  out.samples = std::move(samples);
  out.mode = req.params.mode;
  const size_t n = out.samples.size();
  if (n == 0) value_error(no_sample);
  const size_t rc = in_play.count;
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  out.params = req.as_dict();
  out.has_segments = req.segments;
  out.positions.assign(in_play.positions().begin(), in_play.positions().begin() + (std::ptrdiff_t)rc);
  ibd_summarise(out);  // zero tables of the right shape
  if (rc == 0) return out;
  check_positions_in_play(out.positions, "IBD segments need", "scan");
  out.span(keep, masked);
  if (n == 1 || out.kept_rows == 0) return out;  // no pair or no kept row: nothing for a device to do

  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0;
  if (!dm || rows.rc < rc) throw std::runtime_error("the resident matrix holds fewer rows than are in play");
  const vector<uint32_t> device_x = device_positions(out.positions, dm->variants, r0);
  const size_t words = 4 * n * n;
  DevBuf d_tables(dm->device, words * sizeof(uint64_t));
  unsigned long long* t = (unsigned long long*)d_tables.p;
  const fmh_ibd_out tables{t, t + n * n, t + 2 * n * n, t + 3 * n * n};
  vector<uint64_t> host(words);
  const uint8_t* keep_ptr = masked ? keep.data() : nullptr;
  scan_segments(dm->device, req.segments, n, d_tables, host, out.segments,
                [&](bool with_tables, fmh_ibd_segment* d_segments, size_t capacity, uint64_t* count) {
                  return fmh_ibd_scan(dm->h, out.samples.data(), n, r0, rc, keep_ptr, device_x.data(), &req.params, with_tables ? &tables : nullptr, d_segments,
                                      capacity, count, nullptr);
                },
                fmh_ibd_sort_segments);
  out.n_segments.assign(host.begin(), host.begin() + n * n);
  out.total_sites.assign(host.begin() + n * n, host.begin() + 2 * n * n);
  out.total_length.assign(host.begin() + 2 * n * n, host.begin() + 3 * n * n);
  out.longest.assign(host.begin() + 3 * n * n, host.end());
  return out;
}

void bind_ibd(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<IbdSegments> ibd(m, "IbdSegments");
  bind_segment_result(ibd);
  ibd.def_static("from_segments", &ibd_from_segments, py::arg("samples"), py::arg("segment_a"), py::arg("segment_b"), py::arg("segment_first_row"),
                 py::arg("segment_last_row"), py::arg("segment_sites"), py::arg("segment_missing"), py::arg("positions"),
                 py::arg("sites") = py::none(), py::arg("mode") = "ibd1")
      .def_property_readonly("mode", [](const IbdSegments& r) { return string(r.mode == FMH_IBD2 ? "ibd2" : "ibd1"); })
      .def_property_readonly("n_segments", [](const IbdSegments& r) { return r.table(r.n_segments, r.n()); })
      .def_property_readonly("total_sites", [](const IbdSegments& r) { return r.table(r.total_sites, r.n()); })
      .def_property_readonly("total_length", [](const IbdSegments& r) { return r.table(r.total_length, r.n()); })
      .def_property_readonly("longest", [](const IbdSegments& r) { return r.table(r.longest, r.n()); })
      .def_property_readonly("segment_a", [](const IbdSegments& r) { return r.segment_column<uint32_t>([](const fmh_ibd_segment& s) { return s.a; }); })
      .def_property_readonly("segment_b", [](const IbdSegments& r) { return r.segment_column<uint32_t>([](const fmh_ibd_segment& s) { return s.b; }); })
      .def("ibd_fraction", &IbdSegments::ibd_fraction, py::arg("genome_length") = py::none())
      .def("__len__", &IbdSegments::n)
      .def("__repr__", &IbdSegments::repr);

  m.def("ibd_segments",
        [](const py::object& variants, const py::object& samples, const py::object& sites, const py::object& region, const string& mode, int64_t min_sites,
           int64_t min_length, const py::object& max_gap, const py::object& max_bp_per_site, const py::object& max_missing, bool segments) {
          const IbdRequest req = ibd_parse_request(mode, min_sites, min_length, max_gap, max_bp_per_site, max_missing, segments);
          auto store = store_from_python(variants);
          diploid_only(store->P, (size_t)store->S, "IBD segments take");
          vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
          return ibd_over_rows(rows_in_play(store, region), std::move(list), sites, req, "at least one sample is required for IBD segments");
        },
        py::arg("variants"), py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none(), py::arg("mode") = "ibd1",
        py::arg("min_sites") = 436, py::arg("min_length") = 7000000, py::arg("max_gap") = 1000000, py::arg("max_bp_per_site") = 0,
        py::arg("max_missing") = py::none(), py::arg("segments") = true);
  population.def("ibd_segments",
                 [](const Population& pop, const py::object& sites, const string& mode, int64_t min_sites, int64_t min_length, const py::object& max_gap,
                    const py::object& max_bp_per_site, const py::object& max_missing, bool segments) {
                   const IbdRequest req = ibd_parse_request(mode, min_sites, min_length, max_gap, max_bp_per_site, max_missing, segments);
                   diploid_only(pop, "IBD segments take");
                   return ibd_over_rows(rows_in_play(pop), population_samples(pop), sites, req,
                                        "at least one sample with both haplotypes in the population is required for IBD segments");
                 },
                 py::arg("sites") = py::none(), py::arg("mode") = "ibd1", py::arg("min_sites") = 436, py::arg("min_length") = 7000000,
                 py::arg("max_gap") = 1000000, py::arg("max_bp_per_site") = 0, py::arg("max_missing") = py::none(), py::arg("segments") = true);
}
