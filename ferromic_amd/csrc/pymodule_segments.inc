// pymodule_segments.inc — what the bindings of the segment statistics share (pymodule_roh.inc, pymodule_ibd.inc; the positions in play
// also serve pymodule_clump.inc): the u32 arguments and their None mappings, the positions that go to the library, the part of a result
// that is about its segments, and the two calls that fetch them.  Included inside pymodule_stats.inc's namespace, after pymodule_rows.inc.

// ---- u32 arguments ---------------------------------------------------------------------------------------------------------------------------
uint32_t u32_arg(int64_t v, const char* name) {
  if (v < 0 || v > (int64_t)0xFFFFFFFFll) value_error(string(name) + " must be within 0 .. 2^32 - 1");
  return (uint32_t)v;
}
// None = `none`: 0 for a rule that is off, 2^32 - 1 for a limit that is not set
uint32_t optional_u32_arg(const py::object& o, const char* name, uint32_t none) {
  if (o.is_none()) return none;
  if (!is_intlike(o)) value_error(string(name) + " must be an integer or None");
  const int64_t v = to_i64(o);
  if (v < 0 || v >= (int64_t)0xFFFFFFFFll) value_error(string(name) + " must be within 0 .. 2^32 - 2 or None");
  return (uint32_t)v;
}
py::object none_or_u32(uint32_t v, uint32_t none) { return v == none ? py::object(py::none()) : py::object(py::int_(v)); }

// ---- the positions of the rows in play, as the library takes them -------------------------------------------------------------------------------
// Checked before any device use: `who_needs` ("clumping needs") and `verb` ("clump") word the statistic's refusals.
void check_positions_in_play(const vector<int64_t>& pos, const char* who_needs, const char* verb) {
  for (size_t r = 1; r < pos.size(); ++r)
    if (pos[r] < pos[r - 1]) value_error("the positions descend at variant " + std::to_string(r) + ": " + who_needs + " them in order");
  if (!pos.empty() && (uint64_t)(pos.back() - pos[0]) > 0xFFFFFFFFull)
    value_error("the positions span " + std::to_string(pos.back() - pos[0]) + ", more than 2^32 - 1: " + verb + " one chromosome (or a region of it) at a time");
}
// relative to the first row in play; [variants] of the matrix, of which only the rows of the range, from r0 on, are read
vector<uint32_t> device_positions(const vector<int64_t>& pos, size_t variants, size_t r0) {
  vector<uint32_t> device_x(variants, 0);
  for (size_t r = 0; r < pos.size(); ++r) device_x[r0 + r] = (uint32_t)(pos[r] - pos[0]);
  return device_x;
}

// ---- a result's segments ------------------------------------------------------------------------------------------------------------------------
template <class Segment> struct SegmentResult {
  vector<uint32_t> samples;               // sample numbers, ascending
  uint64_t kept_rows = 0;
  bool has_segments = false, has_span = false;
  vector<Segment> segments;               // in the library's sorted order; rows are rows in play
  vector<int64_t> positions;              // of the rows in play
  int64_t span_first = 0, span_last = 0;  // positions of the first and last kept row (has_span)
  py::object params = py::none();

  void need_segments() const { if (!has_segments) value_error("the result holds no segments: it was computed with segments=False"); }
  template <class T, class F> py::array_t<T> segment_column(F get) const {
    need_segments();
    py::array_t<T> out((py::ssize_t)segments.size());
    for (size_t i = 0; i < segments.size(); ++i) out.mutable_data()[i] = (T)get(segments[i]);
    return out;
  }
  // a [samples][columns] table of the result
  py::array_t<uint64_t> table(const vector<uint64_t>& v, size_t columns) const {
    py::array_t<uint64_t> out({(py::ssize_t)samples.size(), (py::ssize_t)columns});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(uint64_t));
    return out;
  }
  // per row in play: the owners (samples, pairs) with a segment over it (every row of [first_row, last_row]), by a difference array
  py::array_t<uint32_t> site_coverage() const {
    need_segments();
    const size_t rows = positions.size();
    vector<int64_t> diff(rows + 1, 0);
    for (const Segment& s : segments) {
      if (s.last_row >= rows || s.first_row > s.last_row) value_error("a segment lies outside the " + std::to_string(rows) + " rows in play");
      ++diff[s.first_row];
      --diff[s.last_row + 1];
    }
    py::array_t<uint32_t> out((py::ssize_t)rows);
    int64_t depth = 0;
    for (size_t r = 0; r < rows; ++r) { depth += diff[r]; out.mutable_data()[r] = (uint32_t)depth; }
    return out;
  }
  // the kept rows: their number and the span of their positions
  void span(const vector<uint8_t>& keep, bool masked) {
    kept_rows = 0;
    for (size_t r = 0; r < positions.size(); ++r) {
      if (masked && !keep[r]) continue;
      if (!has_span) { has_span = true; span_first = positions[r]; }
      span_last = positions[r];
      ++kept_rows;
    }
  }
  // total_length over the caller's genome_length, else over the span of the kept rows, else NaN; shaped like `shape`
  py::array_t<double> genome_fraction(const vector<uint64_t>& total_length, const py::object& genome_length, vector<py::ssize_t> shape) const {
    double length = has_span ? (double)(span_last - span_first + 1) : std::numeric_limits<double>::quiet_NaN();
    if (!genome_length.is_none()) {
      length = genome_length.cast<double>();
      if (!(length > 0.0)) value_error("genome_length must be positive");
    }
    py::array_t<double> out(shape);
    for (size_t i = 0; i < total_length.size(); ++i) out.mutable_data()[i] = (double)total_length[i] / length;
    return out;
  }
  // from_segments: the positions of the rows, and a segment's rows against them
  void take_positions(const py::object& given) {
    positions = vector_arg<int64_t>(given, "positions", 0, false);
    for (size_t r = 1; r < positions.size(); ++r)
      if (positions[r] < positions[r - 1]) value_error("the positions descend at row " + std::to_string(r));
  }
  void check_segment_rows(size_t i, uint64_t first, uint64_t last) const {
    if (first > last || last >= positions.size()) value_error("segment " + std::to_string(i) + " lies outside the " + std::to_string(positions.size()) + " rows");
  }
};

// the properties every segment result has
template <class Result> void bind_segment_result(py::class_<Result>& c) {
  using Segment = typename decltype(Result::segments)::value_type;
  c.def_property_readonly("samples", [](const Result& r) {
     py::array_t<int64_t> out((py::ssize_t)r.samples.size());
     for (size_t i = 0; i < r.samples.size(); ++i) out.mutable_data()[i] = r.samples[i];
     return out;
   })
      .def_property_readonly("kept_rows", [](const Result& r) { return r.kept_rows; })
      .def_property_readonly("params", [](const Result& r) { return r.params; })
      .def_property_readonly("segment_first_row", [](const Result& r) { return r.template segment_column<uint64_t>([](const Segment& s) { return s.first_row; }); })
      .def_property_readonly("segment_last_row", [](const Result& r) { return r.template segment_column<uint64_t>([](const Segment& s) { return s.last_row; }); })
      .def_property_readonly("segment_start", [](const Result& r) { return r.template segment_column<int64_t>([&r](const Segment& s) { return r.positions[s.first_row]; }); })
      .def_property_readonly("segment_end", [](const Result& r) { return r.template segment_column<int64_t>([&r](const Segment& s) { return r.positions[s.last_row]; }); })
      .def_property_readonly("segment_sites", [](const Result& r) { return r.template segment_column<uint32_t>([](const Segment& s) { return s.n_sites; }); })
      .def_property_readonly("segment_missing", [](const Result& r) { return r.template segment_column<uint32_t>([](const Segment& s) { return s.n_missing; }); })
      .def("site_coverage", [](const Result& r) { return r.site_coverage(); });
}

// The tables and the segments of a scan.  scan(tables, d_segments, capacity, count) makes the C call, with the result's tables only when
// `tables` is set; sort(segments, count) is the library's order.  The first call guesses 64 + 8 n segments; only when the count exceeds the
// guess a second call fetches them into a buffer that holds them all.  The GIL is released around the C calls: scan touches no Python object.
template <class Segment, class Scan, class Sort>
void scan_segments(int dev, bool want_segments, size_t n, const DevBuf& d_tables, vector<uint64_t>& host, vector<Segment>& segments, Scan scan, Sort sort) {
  size_t capacity = want_segments ? 64 + 8 * n : 0;
  uint64_t count = 0;
  std::unique_ptr<DevBuf> d_seg;
  if (want_segments) d_seg = std::make_unique<DevBuf>(dev, capacity * sizeof(Segment));
  int status;
  {
    py::gil_scoped_release nogil;
    status = scan(true, d_seg ? (Segment*)d_seg->p : nullptr, capacity, want_segments ? &count : nullptr);
  }
  fmh_check(status);
  if (count > capacity) {
    capacity = (size_t)count;
    d_seg = std::make_unique<DevBuf>(dev, capacity * sizeof(Segment));
    py::gil_scoped_release nogil;
    status = scan(false, (Segment*)d_seg->p, capacity, &count);
  }
  fmh_check(status);
  {
    py::gil_scoped_release nogil;
    status = fmh_copy_to_host(dev, host.data(), d_tables.p, host.size() * sizeof(uint64_t), nullptr);
    if (status == FMH_OK && count != 0) {
      segments.resize((size_t)count);
      status = fmh_copy_to_host(dev, segments.data(), d_seg->p, (size_t)count * sizeof(Segment), nullptr);
      if (status == FMH_OK) status = sort(segments.data(), segments.size());
    }
  }
  fmh_check(status);
}
