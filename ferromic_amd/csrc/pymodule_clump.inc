// pymodule_clump.inc — ferromic.ld_clump, Population.ld_clump, ferromic.genotype_ld and the Clumps result (included inside
// pymodule_stats.inc's namespace, after pymodule_rows.inc whose rows, sample and sites rules it uses, and pymodule_segments.inc for the positions in play).  An addition to the reference's
// surface: it has no clumping; the definition is include/ferromic_hip.h's (fmh_clump, fmh_geno_ld_pairs, fmh_geno_ld_r2).  Every assignment
// and every r^2 comes from the library; the GIL is released around the C calls.  Positions go to the library relative to the first row in
// play.  A request without a participant or without a candidate, and a genotype_ld of no pair, is answered without a device.

struct Clumps {
  vector<int64_t> index_rows;  // [n_clumps] rows in play, in the order the indexes were chosen (ascending (p, row))
  vector<double> index_p;
  vector<int64_t> clump_sizes;
  vector<int64_t> clump_of, index_of;  // [rows]; -1 for none
  vector<double> r2;                   // [rows]; NaN for none
  vector<int64_t> positions;
  py::object params = py::none();

  size_t n() const { return index_rows.size(); }
  py::array_t<bool> index_mask() const {
    py::array_t<bool> out((py::ssize_t)index_of.size());
    for (size_t r = 0; r < index_of.size(); ++r) out.mutable_data()[r] = index_of[r] == (int64_t)r;
    return out;
  }
  py::array_t<int64_t> members(int64_t k) const {
    if (k < 0 || (size_t)k >= n()) raise(PyExc_IndexError, "clump " + std::to_string(k) + " of " + std::to_string(n()));
    vector<int64_t> rows;
    for (size_t r = 0; r < clump_of.size(); ++r)
      if (clump_of[r] == k) rows.push_back((int64_t)r);
    return array_of(rows);
  }
  string repr() const {
    size_t owned = 0;
    for (int64_t c : clump_of) owned += c >= 0;
    return "Clumps(clumps=" + std::to_string(n()) + ", rows=" + std::to_string(clump_of.size()) + ", assigned=" + std::to_string(owned) + ")";
  }
};

// what the caller asked for, checked before anything is read or uploaded
fmh_clump_params clump_parse_request(double p1, double p2, double r2, int64_t window) {
  fmh_clump_params P{};
  if (std::isnan(p1) || std::isnan(p2) || std::isnan(r2)) value_error("p1, p2 and r2 must not be NaN");
  if (!(0.0 <= p1 && p1 <= p2 && p2 <= 1.0)) value_error("0 <= p1 <= p2 <= 1 is required");
  if (!(0.0 <= r2 && r2 <= 1.0)) value_error("r2 must be within [0, 1]");
  if (window < 0 || window > (int64_t)0xFFFFFFFFll) value_error("window must be within 0 .. 2^32 - 1");
  P.p1 = p1; P.p2 = p2; P.r2 = r2; P.window = (uint32_t)window;
  return P;
}

vector<double> p_values_arg(const py::object& p_values, size_t rows) {
  auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(p_values);
  if (!arr || arr.ndim() != 1) value_error("p_values must be a one-dimensional float array");
  if ((size_t)arr.shape(0) != rows) value_error("p_values has " + std::to_string(arr.shape(0)) + " entries for " + std::to_string(rows) + " rows");
  return vector<double>(arr.data(), arr.data() + rows);
}

Clumps clump_over_rows(const RowsInPlay& in_play, vector<uint32_t> samples, const py::object& sites, const py::object& p_values, const fmh_clump_params& P,
                       const char* no_sample) {
  Clumps out;
  const size_t n = samples.size();
  if (n == 0) value_error(no_sample);
  const size_t rc = in_play.count;
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  const vector<double> p = p_values_arg(p_values, rc);
  py::dict d;
  d["p1"] = P.p1; d["p2"] = P.p2; d["r2"] = P.r2; d["window"] = P.window;
  out.params = d;
  out.positions.assign(in_play.positions().begin(), in_play.positions().begin() + (std::ptrdiff_t)rc);
  out.clump_of.assign(rc, -1);
  out.index_of.assign(rc, -1);
  out.r2.assign(rc, std::numeric_limits<double>::quiet_NaN());
  if (rc == 0) return out;
  // positions relative to the first row in play and the p values, checked before any device use
  check_positions_in_play(out.positions, "clumping needs", "clump");
  size_t participants = 0, candidates = 0;
  for (size_t r = 0; r < rc; ++r) {
    if (masked && !keep[r]) continue;
    if (std::isnan(p[r])) continue;
    if (!(0.0 <= p[r] && p[r] <= 1.0)) value_error("p value " + std::to_string(p[r]) + " of row " + std::to_string(r) + " is neither NaN nor within [0, 1]");
    participants += p[r] <= P.p2;
    candidates += p[r] <= P.p1;
  }
  if (participants == 0 || candidates == 0) return out;  // nothing for a device to do

  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0;
  if (!dm || rows.rc < rc) throw std::runtime_error("the resident matrix holds fewer rows than are in play");
  const vector<uint32_t> device_x = device_positions(out.positions, dm->variants, r0);
  vector<uint32_t> index_of(rc);
  uint64_t n_clumps = 0;
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_clump(dm->h, samples.data(), n, r0, rc, masked ? keep.data() : nullptr, device_x.data(), p.data(), &P, index_of.data(), out.r2.data(), &n_clumps,
                       nullptr);
  }
  fmh_check_args(status);
  // the clumps in the order their indexes were chosen: ascending (p, row)
  for (size_t r = 0; r < rc; ++r)
    if (index_of[r] == (uint32_t)r) out.index_rows.push_back((int64_t)r);
  std::sort(out.index_rows.begin(), out.index_rows.end(), [&](int64_t a, int64_t b) { return p[a] < p[b] || (p[a] == p[b] && a < b); });
  if (out.index_rows.size() != n_clumps) throw std::runtime_error("the library counts " + std::to_string(n_clumps) + " clumps, the assignment holds " + std::to_string(out.index_rows.size()));
  vector<int64_t> number(rc, -1);
  for (size_t k = 0; k < out.index_rows.size(); ++k) {
    number[out.index_rows[k]] = (int64_t)k;
    out.index_p.push_back(p[out.index_rows[k]]);
  }
  out.clump_sizes.assign(out.index_rows.size(), 0);
  for (size_t r = 0; r < rc; ++r) {
    if (index_of[r] == 0xFFFFFFFFu) continue;
    out.index_of[r] = index_of[r];
    out.clump_of[r] = number[index_of[r]];
    ++out.clump_sizes[out.clump_of[r]];
  }
  return out;
}

py::object genotype_ld(const py::object& variants, const py::object& rows_a, const py::object& rows_b, const py::object& samples, const py::object& region,
                       bool counts) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "genotype LD takes");
  vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  const RowsInPlay in_play = rows_in_play(store, region);
  const vector<int64_t> a = vector_arg<int64_t>(rows_a, "rows_a", 0, false);
  const size_t P = a.size();
  const vector<int64_t> b = vector_arg<int64_t>(rows_b, "rows_b", P, true);
  for (size_t i = 0; i < P; ++i)
    if (a[i] < 0 || b[i] < 0 || (size_t)a[i] >= in_play.count || (size_t)b[i] >= in_play.count)
      value_error("pair " + std::to_string(i) + " names rows (" + std::to_string(a[i]) + ", " + std::to_string(b[i]) + ") of " + std::to_string(in_play.count) + " rows in play");
  if (P != 0 && list.empty()) value_error("at least one sample is required for genotype LD");
  py::array_t<double> r2((py::ssize_t)P);
  py::array_t<int64_t> table({(py::ssize_t)P, (py::ssize_t)6});
  if (P != 0) {
    const ResidentRows rows = in_play.resident();
    const shared_ptr<DevMatrix>& dm = rows.dm;
    if (!dm || rows.rc < in_play.count) throw std::runtime_error("the resident matrix holds fewer rows than are in play");
    vector<uint32_t> da(P), db(P);
    for (size_t i = 0; i < P; ++i) { da[i] = (uint32_t)(rows.r0 + a[i]); db[i] = (uint32_t)(rows.r0 + b[i]); }
    DevBuf d_counts(dm->device, P * sizeof(fmh_geno_ld_counts));
    vector<fmh_geno_ld_counts> host(P);
    int status;
    {
      py::gil_scoped_release nogil;
      status = fmh_geno_ld_pairs(dm->h, list.data(), list.size(), da.data(), db.data(), P, (fmh_geno_ld_counts*)d_counts.p, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(dm->device, host.data(), d_counts.p, P * sizeof(fmh_geno_ld_counts), nullptr);
      if (status == FMH_OK) status = fmh_geno_ld_r2(host.data(), P, r2.mutable_data());
    }
    fmh_check_args(status);
    for (size_t i = 0; i < P; ++i) {
      int64_t* row = table.mutable_data() + 6 * i;
      row[0] = host[i].n; row[1] = host[i].sum_a; row[2] = host[i].sum_b; row[3] = host[i].sq_a; row[4] = host[i].sq_b; row[5] = host[i].cross;
    }
  }
  if (counts) return py::make_tuple(r2, table);
  return std::move(r2);
}

void bind_clump(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<Clumps>(m, "Clumps")
      .def_property_readonly("index_rows", [](const Clumps& r) { return array_of(r.index_rows); })
      .def_property_readonly("index_p", [](const Clumps& r) { return array_of(r.index_p); })
      .def_property_readonly("sizes", [](const Clumps& r) { return array_of(r.clump_sizes); })
      .def_property_readonly("clump_of", [](const Clumps& r) { return array_of(r.clump_of); })
      .def_property_readonly("index_of", [](const Clumps& r) { return array_of(r.index_of); })
      .def_property_readonly("r2", [](const Clumps& r) { return array_of(r.r2); })
      .def_property_readonly("positions", [](const Clumps& r) { return array_of(r.positions); })
      .def_property_readonly("params", [](const Clumps& r) { return r.params; })
      .def("index_mask", &Clumps::index_mask)
      .def("members", &Clumps::members, py::arg("k"))
      .def("__len__", &Clumps::n)
      .def("__repr__", &Clumps::repr);

  m.def("ld_clump",
        [](const py::object& variants, const py::object& p_values, const py::object& samples, const py::object& sites, const py::object& region, double p1,
           double p2, double r2, int64_t window) {
          const fmh_clump_params P = clump_parse_request(p1, p2, r2, window);
          auto store = store_from_python(variants);
          diploid_only(store->P, (size_t)store->S, "LD clumping takes");
          vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
          return clump_over_rows(rows_in_play(store, region), std::move(list), sites, p_values, P, "at least one sample is required for LD clumping");
        },
        py::arg("variants"), py::arg("p_values"), py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none(),
        py::arg("p1") = 1e-4, py::arg("p2") = 1e-2, py::arg("r2") = 0.5, py::arg("window") = 250000);
  population.def("ld_clump",
                 [](const Population& pop, const py::object& p_values, const py::object& sites, double p1, double p2, double r2, int64_t window) {
                   const fmh_clump_params P = clump_parse_request(p1, p2, r2, window);
                   diploid_only(pop, "LD clumping takes");
                   return clump_over_rows(rows_in_play(pop), population_samples(pop), sites, p_values, P,
                                          "at least one sample with both haplotypes in the population is required for LD clumping");
                 },
                 py::arg("p_values"), py::arg("sites") = py::none(), py::arg("p1") = 1e-4, py::arg("p2") = 1e-2, py::arg("r2") = 0.5, py::arg("window") = 250000);
  m.def("genotype_ld", &genotype_ld, py::arg("variants"), py::arg("rows_a"), py::arg("rows_b"), py::arg("samples") = py::none(), py::arg("region") = py::none(),
        py::arg("counts") = false);
}
