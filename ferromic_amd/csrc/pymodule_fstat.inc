// pymodule_fstat.inc — ferromic.f_statistics and the classes FStatistics / FStatEstimate (included inside pymodule_stats.inc's namespace,
// after pymodule_sfs.inc whose window parsing, row mapping and population checks it shares).  An addition to the reference's surface: it has
// no f-statistics; the definition is include/ferromic_hip.h's (fmh_fstat_moments, fmh_fstat_f4, fmh_block_jackknife).  The integer moment
// table comes from the device, the GIL is released around the calls; every statistic is fmh_fstat_f4 and fmh_block_jackknife on the host, so
// they work on any table (from_moments, concatenate) without a device.

struct FStatEstimate {
  double estimate, jackknife_estimate, se, z;
  uint64_t blocks, sites;
  string repr() const {
    std::ostringstream os;
    os << "FStatEstimate(estimate=" << estimate << ", se=" << se << ", z=" << z << ", blocks=" << blocks << ", sites=" << sites << ")";
    return os.str();
  }
};

struct FStatistics {
  size_t G = 0, M = 0, n_blocks = 0;
  vector<uint64_t> sizes;                     // [G]
  vector<uint64_t> moments;                   // [n_blocks][M]
  vector<uint64_t> multiallelic, incomplete;  // [n_blocks]

  FStatistics() = default;
  FStatistics(vector<uint64_t> sample_sizes, size_t blocks) : G(sample_sizes.size()), M(fmh_fstat_moment_count((int)sample_sizes.size())),
                                                             n_blocks(blocks), sizes(std::move(sample_sizes)) {
    moments.assign(n_blocks * M, 0);
    multiallelic.assign(n_blocks, 0);
    incomplete.assign(n_blocks, 0);
  }

  py::array_t<uint64_t> moments_array() const {
    py::array_t<uint64_t> out(std::vector<py::ssize_t>{(py::ssize_t)n_blocks, (py::ssize_t)M});
    if (!moments.empty()) memcpy(out.mutable_data(), moments.data(), moments.size() * sizeof(uint64_t));
    return out;
  }
  static py::array_t<uint64_t> per_block(const vector<uint64_t>& t) {
    py::array_t<uint64_t> out((py::ssize_t)t.size());
    if (!t.empty()) memcpy(out.mutable_data(), t.data(), t.size() * sizeof(uint64_t));
    return out;
  }
  py::array_t<uint64_t> usable_array() const {
    py::array_t<uint64_t> out((py::ssize_t)n_blocks);
    for (size_t b = 0; b < n_blocks; ++b) out.mutable_data()[b] = moments[b * M];
    return out;
  }
  py::tuple sizes_tuple() const {
    py::tuple t(G);
    for (size_t g = 0; g < G; ++g) t[g] = py::int_(sizes[g]);
    return t;
  }

  int index(int64_t i) const {
    if (i < 0 || (size_t)i >= G) throw py::index_error("population index " + std::to_string(i) + " is outside 0.." + std::to_string(G - 1));
    return (int)i;
  }
  // the blocks' sums of one f4 estimator
  vector<double> block_sums(int a, int b, int c, int d, bool unbiased) const {
    vector<double> out(n_blocks);
    for (size_t k = 0; k < n_blocks; ++k) fmh_check(fmh_fstat_f4(moments.data() + k * M, sizes.data(), (int)G, a, b, c, d, unbiased ? 1 : 0, &out[k]));
    return out;
  }
  vector<double> usable_f64() const {
    vector<double> out(n_blocks);
    for (size_t k = 0; k < n_blocks; ++k) out[k] = (double)moments[k * M];
    return out;
  }
  uint64_t usable_total() const {
    uint64_t s = 0;
    for (size_t k = 0; k < n_blocks; ++k) s += moments[k * M];
    return s;
  }
  FStatEstimate jackknife(const vector<double>& num, const vector<double>& den, const double* weight) const {
    fmh_jackknife_out o;
    fmh_check(fmh_block_jackknife(num.data(), den.data(), weight, n_blocks, &o));
    return FStatEstimate{o.estimate, o.jackknife_estimate, o.se, o.z, o.blocks, usable_total()};
  }
  FStatEstimate f4(int64_t a, int64_t b, int64_t c, int64_t d, bool unbiased) const {
    const vector<double> num = block_sums(index(a), index(b), index(c), index(d), unbiased);
    return jackknife(num, usable_f64(), nullptr);
  }
  FStatEstimate f2(int64_t a, int64_t b, bool unbiased) const { return f4(a, b, a, b, unbiased); }
  FStatEstimate f3(int64_t c, int64_t a, int64_t b, bool unbiased) const { return f4(c, a, c, b, unbiased); }
  FStatEstimate f4_ratio(const vector<int64_t>& num, const vector<int64_t>& den, bool unbiased) const {
    if (num.size() != 4 || den.size() != 4) value_error("num and den are quadruples of population indices (a, b, c, d)");
    const vector<double> n = block_sums(index(num[0]), index(num[1]), index(num[2]), index(num[3]), unbiased);
    const vector<double> d = block_sums(index(den[0]), index(den[1]), index(den[2]), index(den[3]), unbiased);
    const vector<double> w = usable_f64();
    return jackknife(n, d, w.data());
  }
  // [n_blocks][G][G]: the per-block MEAN of f2 (NaN for a block without a usable row), the layout admixture tools exchange
  py::array_t<double> f2_blocks(bool unbiased) const {
    py::array_t<double> out(std::vector<py::ssize_t>{(py::ssize_t)n_blocks, (py::ssize_t)G, (py::ssize_t)G});
    double* o = out.mutable_data();
    for (size_t k = 0; k < n_blocks; ++k) {
      const double usable = (double)moments[k * M];
      for (size_t i = 0; i < G; ++i)
        for (size_t j = i; j < G; ++j) {
          double sum = 0.0;
          if (i != j) fmh_check(fmh_fstat_f4(moments.data() + k * M, sizes.data(), (int)G, (int)i, (int)j, (int)i, (int)j, unbiased ? 1 : 0, &sum));
          const double mean = moments[k * M] == 0 ? std::numeric_limits<double>::quiet_NaN() : sum / usable;
          o[(k * G + i) * G + j] = o[(k * G + j) * G + i] = mean;
        }
    }
    return out;
  }
  string repr() const { return "FStatistics(populations=" + std::to_string(G) + ", blocks=" + std::to_string(n_blocks) + ")"; }
};

vector<uint64_t> fstat_parse_sizes(const py::object& sample_sizes) {
  vector<uint64_t> sizes;
  for (py::handle s : sample_sizes) {
    if (!is_intlike(s) || to_i64(s) < 1) value_error("sample_sizes must hold positive integers");
    sizes.push_back((uint64_t)to_i64(s));
  }
  if (sizes.size() < 2 || sizes.size() > FMH_FSTAT_MAX_GROUPS) value_error("f-statistics take 2 to 32 populations, got " + std::to_string(sizes.size()));
  return sizes;
}

FStatistics fstat_from_moments(const py::object& obj, const py::object& sample_sizes) {
  vector<uint64_t> sizes = fstat_parse_sizes(sample_sizes);
  auto arr = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>::ensure(obj);
  if (!arr || (arr.ndim() != 1 && arr.ndim() != 2)) value_error("moments must be a 1-D or 2-D array of non-negative integers");
  const size_t M = fmh_fstat_moment_count((int)sizes.size());
  if ((size_t)arr.shape(arr.ndim() - 1) != M)
    value_error("a block's slice has 1 + G + G (G + 1) / 2 = " + std::to_string(M) + " entries for " + std::to_string(sizes.size()) + " populations");
  FStatistics out(std::move(sizes), arr.ndim() == 2 ? (size_t)arr.shape(0) : 1);
  if (!out.moments.empty()) memcpy(out.moments.data(), arr.data(), out.moments.size() * sizeof(uint64_t));
  return out;
}

// per-chromosome results -> one genome-wide set of blocks, in the order given
FStatistics fstat_concatenate(const py::object& parts) {
  vector<const FStatistics*> list;
  for (py::handle p : parts) {
    if (!py::isinstance<FStatistics>(p)) value_error("concatenate takes FStatistics objects");
    list.push_back(p.cast<const FStatistics*>());
  }
  if (list.empty()) value_error("concatenate needs at least one FStatistics");
  FStatistics out(list[0]->sizes, 0);
  for (const FStatistics* p : list) {
    if (p->sizes != out.sizes) value_error("the sample sizes of the parts differ");
    out.moments.insert(out.moments.end(), p->moments.begin(), p->moments.end());
    out.multiallelic.insert(out.multiallelic.end(), p->multiallelic.begin(), p->multiallelic.end());
    out.incomplete.insert(out.incomplete.end(), p->incomplete.begin(), p->incomplete.end());
    out.n_blocks += p->n_blocks;
  }
  return out;
}

FStatistics f_statistics(const py::object& populations, const py::object& blocks, const py::object& block_size) {
  // every argument error before any device use
  if (!blocks.is_none() && !block_size.is_none()) value_error("give blocks or block_size, not both");
  optional<vector<Region>> wins = sfs_parse_windows(blocks);
  int64_t size_bp = 0;
  if (!block_size.is_none()) {
    if (!is_intlike(block_size) || to_i64(block_size) < 1) value_error("block_size must be a positive integer (base pairs)");
    size_bp = to_i64(block_size);
  }
  vector<shared_ptr<Population>> pops;
  for (py::handle p : populations) pops.push_back(coerce_population(p));
  if (pops.size() < 2 || pops.size() > FMH_FSTAT_MAX_GROUPS) value_error("f-statistics take 2 to 32 populations, got " + std::to_string(pops.size()));
  const Population& first = *pops[0];
  for (size_t g = 1; g < pops.size(); ++g) {
    if (!variants_compatible(*first.store, *pops[g]->store)) vcf_error("Parse", "Variant slices differ in positions/length.");
    const bool same_dense = first.dense && first.dense == pops[g]->dense;
    const bool same_store = !first.dense && !pops[g]->dense && first.store == pops[g]->store;
    if (!same_dense && !same_store)
      value_error("the f-statistics need every population over ONE resident matrix: make them with with_haplotypes from one Population");
  }
  const size_t count = first.dense ? (size_t)first.dense->variants : (size_t)first.store->S;
  vector<vector<uint8_t>> masks(pops.size());
  vector<uint64_t> sizes(pops.size());
  for (size_t g = 0; g < pops.size(); ++g) {
    sfs_sample_size(pops[g]->haplotypes, nullptr);
    if (count != 0) {
      masks[g] = population_mask(*pops[g]);
      sizes[g] = sfs_sample_size(pops[g]->haplotypes, &masks[g]);
    } else {
      sizes[g] = pops[g]->haplotypes.size();
    }
  }
  const vector<int64_t>& positions = first.store->positions;
  const size_t rows = std::min(count, positions.size());
  if (size_bp > 0) {  // consecutive windows of block_size base pairs from the first position on
    wins = vector<Region>();
    if (rows != 0) {
      const auto [lo, hi] = std::minmax_element(positions.begin(), positions.begin() + (std::ptrdiff_t)rows);
      const uint64_t n_windows = (uint64_t)(*hi - *lo) / (uint64_t)size_bp + 1;
      if (n_windows > ((uint64_t)1 << 24)) value_error("block_size gives more than 2^24 blocks");
      for (uint64_t w = 0; w < n_windows; ++w) wins->push_back({*lo + (int64_t)w * size_bp, *lo + (int64_t)(w + 1) * size_bp - 1});
    }
  }
  FStatistics out(sizes, wins ? wins->size() : 1);
  if (rows == 0) return out;
  SfsRuns runs;
  if (wins) runs = sfs_runs(positions, rows, 0, *wins);
  else { runs.ranges = {(uint64_t)0, (uint64_t)rows}; runs.window_of = {0}; }
  const size_t n_runs = runs.window_of.size();
  if (n_runs == 0) return out;
  const ResidentRows resident = resident_rows_of(first);
  for (uint64_t& r : runs.ranges) r += resident.r0;
  const DevMatrix& dm = *resident.dm;
  vector<uint8_t> flat;
  flat.reserve(masks.size() * dm.columns());
  for (auto& k : masks) {
    if (k.size() != dm.columns()) value_error("a population's haplotypes do not match the resident matrix's columns");
    flat.insert(flat.end(), k.begin(), k.end());
  }
  const size_t M = out.M;
  DevBuf d_moments(dm.device, n_runs * M * sizeof(uint64_t));
  vector<uint64_t> table(n_runs * M);
  vector<fmh_sfs_skipped> skipped(n_runs);
  int status;
  {
    py::gil_scoped_release nogil;
    status = fmh_fstat_moments(dm.h, flat.data(), (int)masks.size(), runs.ranges.data(), n_runs, (uint64_t*)d_moments.p, skipped.data(), nullptr);
    if (status == FMH_OK) status = fmh_copy_to_host(dm.device, table.data(), d_moments.p, table.size() * sizeof(uint64_t), nullptr);
  }
  fmh_check(status);
  for (size_t r = 0; r < n_runs; ++r) {
    const size_t w = runs.window_of[r];
    for (size_t k = 0; k < M; ++k) out.moments[w * M + k] += table[r * M + k];
    out.multiallelic[w] += skipped[r].multiallelic;
    out.incomplete[w] += skipped[r].incomplete;
  }
  return out;
}

void bind_fstat(py::module_& m) {
  py::class_<FStatEstimate>(m, "FStatEstimate")
      .def_readonly("estimate", &FStatEstimate::estimate)
      .def_readonly("jackknife_estimate", &FStatEstimate::jackknife_estimate)
      .def_readonly("se", &FStatEstimate::se)
      .def_readonly("z", &FStatEstimate::z)
      .def_readonly("blocks", &FStatEstimate::blocks)
      .def_readonly("sites", &FStatEstimate::sites)
      .def("__repr__", &FStatEstimate::repr);
  py::class_<FStatistics>(m, "FStatistics")
      .def_static("from_moments", &fstat_from_moments, py::arg("moments"), py::arg("sample_sizes"))
      .def_static("concatenate", &fstat_concatenate, py::arg("parts"))
      .def_property_readonly("moments", &FStatistics::moments_array)
      .def_property_readonly("sample_sizes", &FStatistics::sizes_tuple)
      .def_property_readonly("usable_sites", &FStatistics::usable_array)
      .def_property_readonly("multiallelic_sites", [](const FStatistics& s) { return FStatistics::per_block(s.multiallelic); })
      .def_property_readonly("incomplete_sites", [](const FStatistics& s) { return FStatistics::per_block(s.incomplete); })
      .def("f2", &FStatistics::f2, py::arg("a"), py::arg("b"), py::arg("unbiased") = true)
      .def("f3", &FStatistics::f3, py::arg("c"), py::arg("a"), py::arg("b"), py::arg("unbiased") = true)
      .def("f4", &FStatistics::f4, py::arg("a"), py::arg("b"), py::arg("c"), py::arg("d"), py::arg("unbiased") = true)
      .def("f4_ratio", &FStatistics::f4_ratio, py::arg("num"), py::arg("den"), py::arg("unbiased") = true)
      .def("f2_blocks", &FStatistics::f2_blocks, py::arg("unbiased") = true)
      .def("__repr__", &FStatistics::repr);
  m.def("f_statistics", &f_statistics, py::arg("populations"), py::arg("blocks") = py::none(), py::arg("block_size") = py::none());
}
