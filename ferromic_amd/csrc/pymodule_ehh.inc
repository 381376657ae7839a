// pymodule_ehh.inc — ferromic.ehh_scan / ihs / nsl, Population.ehh_scan / ihs / nsl and the class HaplotypeScan (included inside
// pymodule_stats.inc's namespace, after pymodule_hap.inc whose haplotype handling it shares).  An addition to the reference's surface; the
// definition is include/ferromic_hip.h's (fmh_ehh_scan, fmh_ehh_stats).  The records come from the device as integers, the GIL is released
// around the C calls; iHH, SL, iHS and nSL are fmh_ehh_stats on the host.

struct HaplotypeScan {
  size_t n = 0;
  vector<uint64_t> focal;         // [F]: rows of the variants (of the region, when one was given)
  vector<fmh_ehh_side> sides;     // [F][2], the left side first
  vector<fmh_ehh_stats_out> stats;  // [F]
  bool has_pairs = false;
  size_t max_extent = 0;
  vector<uint32_t> pairs;         // [F][2][2][max_extent] when has_pairs

  size_t n_focal() const { return focal.size(); }
  py::array_t<uint64_t> focal_rows() const {
    py::array_t<uint64_t> out((py::ssize_t)n_focal());
    if (!focal.empty()) memcpy(out.mutable_data(), focal.data(), focal.size() * sizeof(uint64_t));
    return out;
  }
  py::array_t<uint32_t> core_counts() const {
    py::array_t<uint32_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_focal(), 2});
    for (size_t i = 0; i < n_focal(); ++i)
      for (int a = 0; a < 2; ++a) out.mutable_data()[i * 2 + a] = sides[2 * i].core[a];
    return out;
  }
  // [F][2 sides][2 cores]
  template <typename T, typename Get>
  py::array_t<T> per_side_core(Get get) const {
    py::array_t<T> out(std::vector<py::ssize_t>{(py::ssize_t)n_focal(), 2, 2});
    for (size_t i = 0; i < 2 * n_focal(); ++i)
      for (int a = 0; a < 2; ++a) out.mutable_data()[i * 2 + a] = get(sides[i], a);
    return out;
  }
  py::array_t<uint32_t> flags() const {
    py::array_t<uint32_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_focal(), 2});
    for (size_t i = 0; i < 2 * n_focal(); ++i) out.mutable_data()[i] = sides[i].flags;
    return out;
  }
  py::array_t<double> f64_pair(double (fmh_ehh_stats_out::*field)[2]) const {
    py::array_t<double> out(std::vector<py::ssize_t>{(py::ssize_t)n_focal(), 2});
    for (size_t i = 0; i < n_focal(); ++i)
      for (int a = 0; a < 2; ++a) out.mutable_data()[i * 2 + a] = (stats[i].*field)[a];
    return out;
  }
  py::array_t<double> f64_stat(double fmh_ehh_stats_out::*field) const {
    py::array_t<double> out((py::ssize_t)n_focal());
    for (size_t i = 0; i < n_focal(); ++i) out.mutable_data()[i] = stats[i].*field;
    return out;
  }
  py::object pairs_array() const {
    if (!has_pairs) return py::none();
    py::array_t<uint32_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_focal(), 2, 2, (py::ssize_t)max_extent});
    if (!pairs.empty()) memcpy(out.mutable_data(), pairs.data(), pairs.size() * sizeof(uint32_t));
    return std::move(out);
  }
  string repr() const {
    return "HaplotypeScan(sample_size=" + std::to_string(n) + ", focal=" + std::to_string(n_focal()) + (has_pairs ? ", curve=True" : "") + ")";
  }
};

// what the caller asked for, checked before anything is read or uploaded
struct EhhRequest {
  optional<vector<int64_t>> focal;  // rows of the (region's) variants; none = every row
  fmh_ehh_params params{};
  double min_maf = 0.0;
  bool unit_distance = false, curve = false, include_edges = false;
};
EhhRequest ehh_parse_request(const py::object& focal, double min_ehh, const py::object& max_extent, const py::object& max_gap, double min_maf,
                             bool unit_distance, bool curve, bool include_edges) {
  EhhRequest req;
  if (!focal.is_none()) {
    vector<int64_t> rows;
    for (py::handle h : py::reinterpret_borrow<py::object>(focal)) {
      const py::object o = py::reinterpret_borrow<py::object>(h);
      if (!is_intlike(o)) value_error("focal must hold integers (rows of the variants)");
      const int64_t v = to_i64(o);
      if (v < 0) value_error("focal rows must not be negative");
      rows.push_back(v);
    }
    req.focal = std::move(rows);
  }
  if (!(min_ehh >= 0.0 && min_ehh <= 1.0)) value_error("min_ehh must be within 0 .. 1");
  if (!(min_maf >= 0.0 && min_maf <= 1.0)) value_error("min_maf must be within 0 .. 1");
  auto u32_of = [](const py::object& o, const char* name) -> uint32_t {
    if (o.is_none()) return 0;
    if (!is_intlike(o)) value_error(string(name) + " must be a positive integer or None");
    const int64_t v = to_i64(o);
    if (v <= 0 || v > (int64_t)0xFFFFFFFFll) value_error(string(name) + " must be a positive integer below 2^32 or None");
    return (uint32_t)v;
  };
  req.params.min_ehh_num = (uint32_t)std::llround(min_ehh * 1e6);  // halves away from zero (Python's round() takes them to even)
  req.params.min_ehh_den = 1000000u;
  req.params.max_extent = u32_of(max_extent, "max_extent");
  req.params.max_gap = u32_of(max_gap, "max_gap");
  if (curve && req.params.max_extent == 0) value_error("curve=True needs a max_extent");
  req.min_maf = min_maf;
  req.unit_distance = unit_distance;
  req.curve = curve;
  req.include_edges = include_edges;
  return req;
}

// the rows in play are made resident (the matrix uploaded) only when there is a focal row to scan
HaplotypeScan ehh_over_rows(const HapColumns& cols, EhhRequest req, const RowsInPlay& in_play) {
  HaplotypeScan out;
  const size_t n = cols.n, count = in_play.count;
  const vector<int64_t>& positions = in_play.positions();
  out.n = n;
  out.has_pairs = req.curve;
  out.max_extent = req.params.max_extent;
  if (req.focal) {
    for (int64_t f : *req.focal)
      if ((uint64_t)f >= count) value_error("focal row " + std::to_string(f) + " is outside the " + std::to_string(count) + " variants");
    out.focal.assign(req.focal->begin(), req.focal->end());
  } else {
    out.focal.resize(count);
    for (size_t i = 0; i < count; ++i) out.focal[i] = i;
  }
  vector<uint32_t> x;  // the positions of the rows, checked before any device use
  if (!req.unit_distance) {
    x.resize(count);
    for (size_t i = 0; i < count; ++i) {
      const int64_t p = positions[i];
      if (p < 0 || p > (int64_t)0xFFFFFFFFll) value_error("position " + std::to_string(p) + " is outside 0 .. 2^32 - 1");
      if (i && p < positions[i - 1]) value_error("the positions descend at variant " + std::to_string(i) + ": a haplotype scan needs them in order");
      x[i] = (uint32_t)p;
    }
  }
  req.params.min_core = (uint32_t)std::ceil(req.min_maf * (double)n);
  const size_t F = out.focal.size();
  if (req.curve && F > ((size_t)1 << 32) / 4 / out.max_extent) value_error("a curve of " + std::to_string(F) + " focal rows x " + std::to_string(out.max_extent) + " steps exceeds 2^32 entries");
  out.sides.resize(2 * F);
  out.stats.resize(F);
  if (req.curve) out.pairs.assign(F * 4 * out.max_extent, 0);
  if (F) {
    const ResidentRows rows = in_play.resident(cols.mask);
    const DevMatrix& dm = *rows.dm;
    vector<uint64_t> device_focal = out.focal;
    for (uint64_t& f : device_focal) f += rows.r0;
    vector<uint32_t> device_x;  // [variants] of the matrix: only the rows of the range are read
    if (!req.unit_distance) {
      device_x.assign(dm.variants, 0);
      std::copy(x.begin(), x.end(), device_x.begin() + (std::ptrdiff_t)rows.r0);
    }
    const shared_ptr<Groups> gp = groups_for(dm, {rows.mask});
    DevBuf d_out(dm.device, out.sides.size() * sizeof(fmh_ehh_side));
    std::unique_ptr<DevBuf> d_pairs;
    if (req.curve) d_pairs = std::make_unique<DevBuf>(dm.device, std::max<size_t>(out.pairs.size(), 1) * sizeof(uint32_t));
    int status;
    {
      py::gil_scoped_release nogil;
      status = fmh_ehh_scan(dm.h, gp->h, rows.r0, rows.r0 + count, device_focal.data(), F, req.unit_distance ? nullptr : device_x.data(), &req.params,
                            (fmh_ehh_side*)d_out.p, d_pairs ? (uint32_t*)d_pairs->p : nullptr, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dm.device, out.sides.data(), d_out.p, out.sides.size() * sizeof(fmh_ehh_side), nullptr);
      if (status == FMH_OK && req.curve && !out.pairs.empty())
        status = fmh_copy_to_host(dm.device, out.pairs.data(), d_pairs->p, out.pairs.size() * sizeof(uint32_t), nullptr);
    }
    fmh_check(status);
    {
      py::gil_scoped_release nogil;
      status = fmh_ehh_stats(out.sides.data(), F, req.include_edges ? 1 : 0, out.stats.data());
    }
    fmh_check(status);
  }
  return out;
}

HaplotypeScan ehh_of_variants(const py::object& variants, const py::object& haplotypes, const py::object& region, const EhhRequest& req) {
  const vector<Hap> haps = parse_haplotypes(haplotypes);
  hap_sample_size(haps, nullptr);
  const optional<Region> reg = region_arg(region);
  auto store = store_from_python(variants);
  const HapColumns cols = hap_columns(*store, haps, hap_sample_size);
  return ehh_over_rows(cols, req, rows_in_play(store, reg));
}

HaplotypeScan ehh_of_population(const Population& pop, const EhhRequest& req) {
  hap_sample_size(pop.haplotypes, nullptr);
  return ehh_over_rows(hap_columns(pop, hap_sample_size), req, rows_in_play(pop));
}

void bind_ehh(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<HaplotypeScan>(m, "HaplotypeScan")
      .def_property_readonly("sample_size", [](const HaplotypeScan& h) { return h.n; })
      .def_property_readonly("focal_rows", &HaplotypeScan::focal_rows)
      .def_property_readonly("core_counts", &HaplotypeScan::core_counts)
      .def_property_readonly("area2", [](const HaplotypeScan& h) { return h.per_side_core<uint64_t>([](const fmh_ehh_side& s, int a) { return s.area2[a]; }); })
      .def_property_readonly("pair_steps", [](const HaplotypeScan& h) { return h.per_side_core<uint64_t>([](const fmh_ehh_side& s, int a) { return s.pair_steps[a]; }); })
      .def_property_readonly("steps", [](const HaplotypeScan& h) { return h.per_side_core<uint32_t>([](const fmh_ehh_side& s, int a) { return s.steps[a]; }); })
      .def_property_readonly("flags", &HaplotypeScan::flags)
      .def_property_readonly("ihh", [](const HaplotypeScan& h) { return h.f64_pair(&fmh_ehh_stats_out::ihh); })
      .def_property_readonly("sl", [](const HaplotypeScan& h) { return h.f64_pair(&fmh_ehh_stats_out::sl); })
      .def_property_readonly("ihs", [](const HaplotypeScan& h) { return h.f64_stat(&fmh_ehh_stats_out::ihs); })
      .def_property_readonly("nsl", [](const HaplotypeScan& h) { return h.f64_stat(&fmh_ehh_stats_out::nsl); })
      .def_property_readonly("pairs", &HaplotypeScan::pairs_array)
      .def("__len__", &HaplotypeScan::n_focal)
      .def("__repr__", &HaplotypeScan::repr);

  // ehh_scan: everything is the caller's; ihs: positions, threshold 0.05, minor core 0.05 n; nsl: unit distance, no threshold, 100 rows, edges kept
  m.def("ehh_scan",
        [](const py::object& variants, const py::object& haplotypes, const py::object& region, const py::object& focal, double min_ehh,
           const py::object& max_extent, const py::object& max_gap, double min_maf, bool unit_distance, bool curve, bool include_edges) {
          return ehh_of_variants(variants, haplotypes, region, ehh_parse_request(focal, min_ehh, max_extent, max_gap, min_maf, unit_distance, curve, include_edges));
        },
        py::arg("variants"), py::arg("haplotypes"), py::arg("region") = py::none(), py::arg("focal") = py::none(), py::arg("min_ehh") = 0.05,
        py::arg("max_extent") = py::none(), py::arg("max_gap") = py::none(), py::arg("min_maf") = 0.0, py::arg("unit_distance") = false,
        py::arg("curve") = false, py::arg("include_edges") = false);
  m.def("ihs",
        [](const py::object& variants, const py::object& haplotypes, const py::object& region, const py::object& focal, double min_ehh,
           const py::object& max_extent, const py::object& max_gap, double min_maf, bool include_edges) {
          return ehh_of_variants(variants, haplotypes, region, ehh_parse_request(focal, min_ehh, max_extent, max_gap, min_maf, false, false, include_edges));
        },
        py::arg("variants"), py::arg("haplotypes"), py::arg("region") = py::none(), py::arg("focal") = py::none(), py::arg("min_ehh") = 0.05,
        py::arg("max_extent") = py::none(), py::arg("max_gap") = py::none(), py::arg("min_maf") = 0.05, py::arg("include_edges") = false);
  m.def("nsl",
        [](const py::object& variants, const py::object& haplotypes, const py::object& region, const py::object& focal, const py::object& max_extent,
           double min_maf) {
          return ehh_of_variants(variants, haplotypes, region, ehh_parse_request(focal, 0.0, max_extent, py::none(), min_maf, true, false, true));
        },
        py::arg("variants"), py::arg("haplotypes"), py::arg("region") = py::none(), py::arg("focal") = py::none(), py::arg("max_extent") = 100,
        py::arg("min_maf") = 0.0);
  population
      .def("ehh_scan",
           [](const Population& pop, const py::object& focal, double min_ehh, const py::object& max_extent, const py::object& max_gap, double min_maf,
              bool unit_distance, bool curve, bool include_edges) {
             return ehh_of_population(pop, ehh_parse_request(focal, min_ehh, max_extent, max_gap, min_maf, unit_distance, curve, include_edges));
           },
           py::arg("focal") = py::none(), py::arg("min_ehh") = 0.05, py::arg("max_extent") = py::none(), py::arg("max_gap") = py::none(),
           py::arg("min_maf") = 0.0, py::arg("unit_distance") = false, py::arg("curve") = false, py::arg("include_edges") = false)
      .def("ihs",
           [](const Population& pop, const py::object& focal, double min_ehh, const py::object& max_extent, const py::object& max_gap, double min_maf,
              bool include_edges) {
             return ehh_of_population(pop, ehh_parse_request(focal, min_ehh, max_extent, max_gap, min_maf, false, false, include_edges));
           },
           py::arg("focal") = py::none(), py::arg("min_ehh") = 0.05, py::arg("max_extent") = py::none(), py::arg("max_gap") = py::none(),
           py::arg("min_maf") = 0.05, py::arg("include_edges") = false)
      .def("nsl",
           [](const Population& pop, const py::object& focal, const py::object& max_extent, double min_maf) {
             return ehh_of_population(pop, ehh_parse_request(focal, 0.0, max_extent, py::none(), min_maf, true, false, true));
           },
           py::arg("focal") = py::none(), py::arg("max_extent") = 100, py::arg("min_maf") = 0.0);
}
