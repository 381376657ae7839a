// pymodule_ibd.inc — ferromic.ibd_segments, Population.ibd_segments and the IbdSegments result (included inside pymodule_stats.inc's
// namespace, after pymodule_rows.inc whose rows, sample and sites rules it uses).  An addition to the reference's surface: it has no IBD
// segments; the definition is include/ferromic_hip.h's (fmh_ibd_scan, fmh_ibd_sort_segments).  Every integer comes from the device; the IBD
// fraction and the coverage track are computed from them on the host; the GIL is released around the C calls.  Positions go to the library
// relative to the first row in play.  A request with one sample or without a kept row is answered without a device.

struct IbdSegments {
  vector<uint32_t> samples;                                        // sample numbers, ascending
  vector<uint64_t> n_segments, total_sites, total_length, longest;  // [n][n]
  uint32_t mode = FMH_IBD1;
  uint64_t kept_rows = 0;
  bool has_segments = false, has_span = false;
  vector<fmh_ibd_segment> segments;                                // sorted by (a, b, first_row); rows are rows in play
  vector<int64_t> positions;                                       // of the rows in play
  int64_t span_first = 0, span_last = 0;                           // positions of the first and last kept row (has_span)
  py::object params = py::none();

  size_t n() const { return samples.size(); }
  void need_segments() const { if (!has_segments) value_error("the result holds no segments: it was computed with segments=False"); }
  template <class T, class F> py::array_t<T> segment_column(F get) const {
    need_segments();
    py::array_t<T> out((py::ssize_t)segments.size());
    for (size_t i = 0; i < segments.size(); ++i) out.mutable_data()[i] = (T)get(segments[i]);
    return out;
  }
  py::array_t<uint64_t> square(const vector<uint64_t>& v) const {
    py::array_t<uint64_t> out({(py::ssize_t)n(), (py::ssize_t)n()});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(uint64_t));
    return out;
  }
  py::array_t<double> ibd_fraction(const py::object& genome_length) const {
    double length = std::numeric_limits<double>::quiet_NaN();
    if (!genome_length.is_none()) {
      length = genome_length.cast<double>();
      if (!(length > 0.0)) value_error("genome_length must be positive");
    } else if (has_span) length = (double)(span_last - span_first + 1);
    py::array_t<double> out({(py::ssize_t)n(), (py::ssize_t)n()});
    for (size_t i = 0; i < n() * n(); ++i) out.mutable_data()[i] = (double)total_length[i] / length;
    return out;
  }
  // per row in play: the pairs with a qualifying segment over it (every row of [first_row, last_row]), by a difference array
  py::array_t<uint32_t> site_coverage() const {
    need_segments();
    const size_t rows = positions.size();
    vector<int64_t> diff(rows + 1, 0);
    for (const fmh_ibd_segment& s : segments) {
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
    auto limit = [](uint32_t v) -> py::object { return v == 0xFFFFFFFFu ? py::object(py::none()) : py::object(py::int_(v)); };
    auto unless_zero = [](uint32_t v) -> py::object { return v == 0 ? py::object(py::none()) : py::object(py::int_(v)); };
    d["mode"] = params.mode == FMH_IBD2 ? "ibd2" : "ibd1";
    d["min_sites"] = params.min_sites; d["min_length"] = params.min_length;
    d["max_gap"] = unless_zero(params.max_gap); d["max_bp_per_site"] = unless_zero(params.max_bp_per_site);
    d["max_missing"] = limit(params.max_missing);
    return d;
  }
};
IbdRequest ibd_parse_request(const string& mode, int64_t min_sites, int64_t min_length, const py::object& max_gap, const py::object& max_bp_per_site,
                             const py::object& max_missing, bool segments) {
  IbdRequest req;
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
  req.params.mode = ibd_mode_arg(mode);
  req.params.min_sites = u32_of(min_sites, "min_sites");
  req.params.min_length = u32_of(min_length, "min_length");
  req.params.max_gap = optional_u32(max_gap, "max_gap", 0);
  req.params.max_bp_per_site = optional_u32(max_bp_per_site, "max_bp_per_site", 0);
  req.params.max_missing = optional_u32(max_missing, "max_missing", 0xFFFFFFFFu);
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

// the span of the kept rows and their number
void ibd_span(IbdSegments& out, const vector<uint8_t>& keep, bool masked) {
  out.kept_rows = 0;
  for (size_t r = 0; r < out.positions.size(); ++r) {
    if (masked && !keep[r]) continue;
    if (!out.has_span) { out.has_span = true; out.span_first = out.positions[r]; }
    out.span_last = out.positions[r];
    ++out.kept_rows;
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
  out.positions = vector_arg<int64_t>(positions, "positions", 0, false);
  const size_t rows = out.positions.size();
  for (size_t r = 1; r < rows; ++r)
    if (out.positions[r] < out.positions[r - 1]) value_error("the positions descend at row " + std::to_string(r));
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rows, &masked);
  out.has_segments = true;
  out.segments.resize(count);
  for (size_t i = 0; i < count; ++i) {
    if (a[i] >= b[i] || b[i] >= out.samples.size())
      value_error("segment " + std::to_string(i) + " names the pair (" + std::to_string(a[i]) + ", " + std::to_string(b[i]) + ") of " + std::to_string(out.samples.size()) + " samples: a < b < n is required");
    if (first[i] > last[i] || last[i] >= rows) value_error("segment " + std::to_string(i) + " lies outside the " + std::to_string(rows) + " rows");
    out.segments[i] = fmh_ibd_segment{a[i], b[i], n_sites[i], n_missing[i], first[i], last[i]};
  }
  fmh_check_args(fmh_ibd_sort_segments(out.segments.data(), count));
  ibd_span(out, keep, masked);
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
  // positions relative to the first row in play, checked before any device use
  const vector<int64_t>& pos = out.positions;
  for (size_t r = 1; r < rc; ++r)
    if (pos[r] < pos[r - 1]) value_error("the positions descend at variant " + std::to_string(r) + ": IBD segments need them in order");
  if ((uint64_t)(pos[rc - 1] - pos[0]) > 0xFFFFFFFFull)
    value_error("the positions span " + std::to_string(pos[rc - 1] - pos[0]) + ", more than 2^32 - 1: scan one chromosome (or a region of it) at a time");
  ibd_span(out, keep, masked);
  if (n == 1 || out.kept_rows == 0) return out;  // no pair or no kept row: nothing for a device to do

  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0;
  if (!dm || rows.rc < rc) throw std::runtime_error("the resident matrix holds fewer rows than are in play");
  vector<uint32_t> device_x(dm->variants, 0);  // [variants] of the matrix: only the rows of the range are read
  for (size_t r = 0; r < rc; ++r) device_x[r0 + r] = (uint32_t)(pos[r] - pos[0]);
  const size_t words = 4 * n * n;
  DevBuf d_tables(dm->device, words * sizeof(uint64_t));
  unsigned long long* t = (unsigned long long*)d_tables.p;
  const fmh_ibd_out tables{t, t + n * n, t + 2 * n * n, t + 3 * n * n};
  vector<uint64_t> host(words);
  size_t capacity = req.segments ? 64 + 8 * n : 0;  // the first guess; a second call only when the segments outnumber it
  uint64_t count = 0;
  const int dev = dm->device;
  const uint8_t* keep_ptr = masked ? keep.data() : nullptr;
  std::unique_ptr<DevBuf> d_seg;
  if (req.segments) d_seg = std::make_unique<DevBuf>(dev, capacity * sizeof(fmh_ibd_segment));
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_ibd_scan(dm->h, out.samples.data(), n, r0, rc, keep_ptr, device_x.data(), &req.params, &tables, d_seg ? (fmh_ibd_segment*)d_seg->p : nullptr,
                          capacity, req.segments ? &count : nullptr, nullptr);
  }
  fmh_check(status);
  if (count > capacity) {  // the guess was short: the segments again, into a buffer that holds them all
    capacity = (size_t)count;
    d_seg = std::make_unique<DevBuf>(dev, capacity * sizeof(fmh_ibd_segment));
    py::gil_scoped_release nogil;
    status = fmh_ibd_scan(dm->h, out.samples.data(), n, r0, rc, keep_ptr, device_x.data(), &req.params, nullptr, (fmh_ibd_segment*)d_seg->p, capacity, &count, nullptr);
  }
  fmh_check(status);
  {
    py::gil_scoped_release nogil;
    status = fmh_copy_to_host(dev, host.data(), d_tables.p, words * sizeof(uint64_t), nullptr);
    if (status == FMH_OK && count != 0) {
      out.segments.resize((size_t)count);
      status = fmh_copy_to_host(dev, out.segments.data(), d_seg->p, (size_t)count * sizeof(fmh_ibd_segment), nullptr);
      if (status == FMH_OK) status = fmh_ibd_sort_segments(out.segments.data(), out.segments.size());
    }
  }
  fmh_check(status);
  out.n_segments.assign(host.begin(), host.begin() + n * n);
  out.total_sites.assign(host.begin() + n * n, host.begin() + 2 * n * n);
  out.total_length.assign(host.begin() + 2 * n * n, host.begin() + 3 * n * n);
  out.longest.assign(host.begin() + 3 * n * n, host.end());
  return out;
}

void bind_ibd(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<IbdSegments>(m, "IbdSegments")
      .def_static("from_segments", &ibd_from_segments, py::arg("samples"), py::arg("segment_a"), py::arg("segment_b"), py::arg("segment_first_row"),
                  py::arg("segment_last_row"), py::arg("segment_sites"), py::arg("segment_missing"), py::arg("positions"),
                  py::arg("sites") = py::none(), py::arg("mode") = "ibd1")
      .def_property_readonly("samples", [](const IbdSegments& r) {
        py::array_t<int64_t> out((py::ssize_t)r.samples.size());
        for (size_t i = 0; i < r.samples.size(); ++i) out.mutable_data()[i] = r.samples[i];
        return out;
      })
      .def_property_readonly("mode", [](const IbdSegments& r) { return string(r.mode == FMH_IBD2 ? "ibd2" : "ibd1"); })
      .def_property_readonly("n_segments", [](const IbdSegments& r) { return r.square(r.n_segments); })
      .def_property_readonly("total_sites", [](const IbdSegments& r) { return r.square(r.total_sites); })
      .def_property_readonly("total_length", [](const IbdSegments& r) { return r.square(r.total_length); })
      .def_property_readonly("longest", [](const IbdSegments& r) { return r.square(r.longest); })
      .def_property_readonly("kept_rows", [](const IbdSegments& r) { return r.kept_rows; })
      .def_property_readonly("params", [](const IbdSegments& r) { return r.params; })
      .def_property_readonly("segment_a", [](const IbdSegments& r) { return r.segment_column<uint32_t>([](const fmh_ibd_segment& s) { return s.a; }); })
      .def_property_readonly("segment_b", [](const IbdSegments& r) { return r.segment_column<uint32_t>([](const fmh_ibd_segment& s) { return s.b; }); })
      .def_property_readonly("segment_first_row", [](const IbdSegments& r) { return r.segment_column<uint64_t>([](const fmh_ibd_segment& s) { return s.first_row; }); })
      .def_property_readonly("segment_last_row", [](const IbdSegments& r) { return r.segment_column<uint64_t>([](const fmh_ibd_segment& s) { return s.last_row; }); })
      .def_property_readonly("segment_start", [](const IbdSegments& r) { return r.segment_column<int64_t>([&r](const fmh_ibd_segment& s) { return r.positions[s.first_row]; }); })
      .def_property_readonly("segment_end", [](const IbdSegments& r) { return r.segment_column<int64_t>([&r](const fmh_ibd_segment& s) { return r.positions[s.last_row]; }); })
      .def_property_readonly("segment_sites", [](const IbdSegments& r) { return r.segment_column<uint32_t>([](const fmh_ibd_segment& s) { return s.n_sites; }); })
      .def_property_readonly("segment_missing", [](const IbdSegments& r) { return r.segment_column<uint32_t>([](const fmh_ibd_segment& s) { return s.n_missing; }); })
      .def("ibd_fraction", &IbdSegments::ibd_fraction, py::arg("genome_length") = py::none())
      .def("site_coverage", &IbdSegments::site_coverage)
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
