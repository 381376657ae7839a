// pymodule_pca.inc — ferromic.chromosome_pca / chromosome_pca_to_file / per_chromosome_pca and ChromosomePcaResult (included inside
// pymodule_stats.inc's namespace).  Mirrors src/lib.rs:195-257, 1780-2156 (coercions, validation order, error texts) and
// src/pca.rs:46-413 (the site filter, on the host from the device scan's integer counts), :846-1103 (the TSV writer and the combiner).
// The pipeline after parsing is pca_host.hpp's (shared with run_vcf): the standardised Gram and the eigenproblem run behind the C-ABI
// (fmh_pca_*); the GIL is released around them.
// (needs <cerrno>, <filesystem>, <fstream>, <sstream> and pca_host.hpp: pymodule.cpp includes them)
struct ChromosomePcaResult {  // lib.rs:195-257
  vector<string> haplotype_labels;
  py::array_t<double> coordinates;
  py::array_t<int64_t> positions;
  string repr() const {
    return "ChromosomePcaResult(haplotypes=" + std::to_string(coordinates.shape(0)) + ", components=" + std::to_string(coordinates.shape(1)) +
           ", variants=" + std::to_string(positions.shape(0)) + ")";
  }
};

// One call's cohort on the host, one byte per entry: 0, 1, 2 for ANY allele above 1 (the filter only asks "above 1"), kPcaMissing.
constexpr uint8_t kPcaMissing = 0xFF;
struct PcaInput {
  size_t variants = 0, samples = 0;
  vector<uint8_t> data;  // [variants][samples][2]
  vector<int64_t> positions;
  // compute_chromosome_pca (Variant input, pca.rs:93-117) counts a complete site with an allele above 1 as complete;
  // compute_chromosome_pca_from_dense (:261-268, :311-315) does not
  bool variant_rule = false;
  void resize(size_t v, size_t s) { variants = v; samples = s; data.assign(v * s * 2, 0); }
  void set(size_t idx, long long value) { data[idx] = value < 0 ? kPcaMissing : (uint8_t)(value > 1 ? 2 : value); }
};

typedef fmpca::Output PcaOutput;

// The pipeline after parsing (pca_host.hpp, shared with run_vcf) on one matrix on the current device.  false = the reference's
// VcfError::Parse with `*parse_error`; device failures raise RuntimeError.
bool pca_compute(PcaInput& in, size_t n_components, PcaOutput* out, string* parse_error) {
  const size_t S = in.variants;
  if (S == 0) { out->haplotypes = in.samples * 2; *parse_error = in.variant_rule ? "No variants provided for PCA" : "No variants with MAF >= 5% found for PCA"; return false; }
  const int device = current_device();
  // the missing bitset of fmh_matrix_create (one bit per entry) straight from the sentinel, which becomes 0
  bool any_missing = false;
  vector<uint64_t> words((in.data.size() + 63) / 64, 0);
  uint8_t max_allele = 0;
  for (size_t i = 0; i < in.data.size(); ++i) {
    if (in.data[i] == kPcaMissing) { words[i >> 6] |= 1ull << (i & 63); in.data[i] = 0; any_missing = true; }
    else max_allele = std::max(max_allele, in.data[i]);
  }
  int rc = FMH_OK;
  string device_error;
  bool ok = true;
  {
    py::gil_scoped_release nogil;
    fmh_matrix* mh = nullptr;
    try {
      fmpca::check(fmh_matrix_create(in.data.data(), any_missing ? words.data() : nullptr, S, in.samples, 2, max_allele, device, &mh));
      fmpca::SlabInput slab;
      slab.m = mh; slab.device = device; slab.rows = S;
      ok = fmpca::compute({slab}, in.samples, in.positions.data(), n_components, in.variant_rule, [](auto&& fn) { fn((size_t)0); }, out, parse_error);
    } catch (const fmpca::DeviceError& e) {
      rc = e.status;
      device_error = e.what();
    }
    if (mh) (void)fmh_matrix_destroy(mh);
  }
  if (rc != FMH_OK) raise(PyExc_RuntimeError, "libferromic_hip status " + std::to_string(rc) + ": " + device_error);
  return ok;
}

// ---- input coercion ---------------------------------------------------------------------------------------------------------------
// i16 extraction as PyO3's: ints (numpy integers, bools) in range
bool pca_extract_i16(const py::handle& o, long long* out) {
  if (!PyLong_Check(o.ptr()) && !is_np_integer(o)) return false;
  int overflow = 0;
  const long long v = PyLong_AsLongLongAndOverflow(py::int_(py::reinterpret_borrow<py::object>(o)).ptr(), &overflow);
  if (overflow || v < -32768 || v > 32767) return false;
  *out = v;
  return true;
}
long long pca_require_i16(const py::handle& o) {
  long long v = 0;
  if (!PyLong_Check(o.ptr()) && !is_np_integer(o)) raise(PyExc_TypeError, "allele must be an integer");
  if (!pca_extract_i16(o, &v)) raise(PyExc_OverflowError, "out of range integral type conversion attempted");
  return v;
}

// extract_diploid_alleles, lib.rs:1951-1997; false = the call does not parse (the caller falls back to the Variant route)
bool pca_diploid_alleles(const py::handle& call, long long* left, long long* right) {
  *left = *right = -1;
  if (call.is_none()) return true;
  long long v = 0;
  if (pca_extract_i16(call, &v)) { *left = *right = v; return true; }
  if (PyList_Check(call.ptr()) || PyTuple_Check(call.ptr())) {
    py::sequence s = py::reinterpret_borrow<py::sequence>(call);
    if (s.size() < 2) return true;
    *left = pca_require_i16(s[0]);
    *right = pca_require_i16(s[1]);
    return true;
  }
  PyObject* it = PyObject_GetIter(call.ptr());
  if (!it) { PyErr_Clear(); return false; }
  py::object iter = py::reinterpret_steal<py::object>(it);
  long long alleles[2] = {0, 0};
  int count = 0;
  while (count < 2) {
    PyObject* a = PyIter_Next(iter.ptr());
    if (!a) { if (PyErr_Occurred()) throw py::error_already_set(); break; }
    py::object allele = py::reinterpret_steal<py::object>(a);
    alleles[count++] = pca_require_i16(allele);
  }
  if (count == 2) { *left = alleles[0]; *right = alleles[1]; }
  return true;
}

// dense_variant_components, lib.rs:1924-1949
std::pair<int64_t, py::object> pca_variant_components(const py::handle& entry) {
  if (py::isinstance<py::tuple>(entry)) {
    py::tuple t = py::reinterpret_borrow<py::tuple>(entry);
    if (t.size() != 2) value_error("variant tuples must have length 2: (position, genotypes)");
    return {to_i64(t[0]), py::object(t[1])};
  }
  if (py::isinstance<py::dict>(entry)) {
    py::dict d = py::reinterpret_borrow<py::dict>(entry);
    const int64_t pos = to_i64(mapping_field(d, {"position", "pos", "site"}));
    return {pos, mapping_field(d, {"genotypes", "calls"})};
  }
  py::object position = field(entry, {"position", "pos", "site"});
  if (position.is_none()) value_error("variant is missing a position");
  py::object genotypes = field(entry, {"genotypes", "calls"});
  if (genotypes.is_none()) value_error("variant is missing genotypes");
  return {to_i64(position), genotypes};
}

// the dict form {"genotypes": (V, S, 2) int16 / int8 / uint8 / uint16, "positions": ...}: lib.rs:1843-1862, 1999-2040 and the
// checks of compute_chromosome_pca_from_dense (pca.rs:218-242), all before any device work
void pca_input_from_mapping(const py::dict& mapping, size_t expected_samples, PcaInput* in) {
  py::object genotypes = mapping["genotypes"];
  if (!mapping.contains("positions")) value_error("dense chromosome PCA input requires a 'positions' array");
  static const char* kMsg = "genotypes must be a numpy.ndarray with dtype int16/int8/uint8/uint16 and shape (variants, samples, ploidy)";
  if (!py::isinstance<py::array>(genotypes)) value_error(kMsg);
  py::array arr = py::reinterpret_borrow<py::array>(genotypes);
  const py::dtype dt = arr.dtype();
  const bool u8 = dt.is(py::dtype::of<uint8_t>()), i8 = dt.is(py::dtype::of<int8_t>()), u16 = dt.is(py::dtype::of<uint16_t>()),
             i16 = dt.is(py::dtype::of<int16_t>());
  if (arr.ndim() != 3 || !(u8 || i8 || u16 || i16)) value_error(kMsg);
  const size_t V = (size_t)arr.shape(0), N = (size_t)arr.shape(1), P = (size_t)arr.shape(2);
  const py::ssize_t s0 = arr.strides(0), s1 = arr.strides(1), s2 = arr.strides(2);
  const char* base = static_cast<const char*>(arr.data());
  if (u16) {
    for (size_t v = 0; v < V; ++v) for (size_t s = 0; s < N; ++s) for (size_t k = 0; k < P; ++k) {
      uint16_t x; memcpy(&x, base + (py::ssize_t)v * s0 + (py::ssize_t)s * s1 + (py::ssize_t)k * s2, 2);
      if (x > 32767) value_error("allele values must fit within signed 16-bit integers");
    }
  }
  vector<int64_t> positions = extract_positions(mapping["positions"], (int64_t)V);
  if (N != expected_samples)
    vcf_error("Parse", "genotype sample dimension " + std::to_string(N) + " does not match sample_names length " + std::to_string(expected_samples));
  if (P != 2) vcf_error("Parse", "expected diploid genotypes (ploidy=2) but received ploidy " + std::to_string(P));
  in->resize(V, N);
  in->positions = std::move(positions);
  for (size_t v = 0; v < V; ++v) for (size_t s = 0; s < N; ++s) for (size_t k = 0; k < 2; ++k) {
    const char* q = base + (py::ssize_t)v * s0 + (py::ssize_t)s * s1 + (py::ssize_t)k * s2;  // any strides: no contiguous copy first
    long long x;
    if (u8) { uint8_t t; memcpy(&t, q, 1); x = t; } else if (i8) { int8_t t; memcpy(&t, q, 1); x = t; }
    else if (u16) { uint16_t t; memcpy(&t, q, 2); x = t; } else { int16_t t; memcpy(&t, q, 2); x = t; }
    in->set((v * N + s) * 2 + k, x);
  }
}

// try_parse_variant_sequence_to_dense, lib.rs:1871-1922: a LIST of records whose genotypes are lists and whose calls all parse
bool pca_input_from_list(const py::list& list, size_t expected_samples, PcaInput* in) {
  const size_t V = list.size();
  in->resize(V, expected_samples);
  in->positions.resize(V);
  for (size_t v = 0; v < V; ++v) {
    auto [position, genotypes] = pca_variant_components(list[v]);
    if (!PyList_Check(genotypes.ptr())) return false;
    py::list calls = py::reinterpret_borrow<py::list>(genotypes);
    if (calls.size() != expected_samples)
      value_error("variant " + std::to_string(v) + " contains " + std::to_string(calls.size()) + " samples but " + std::to_string(expected_samples) +
                  " names were provided");
    in->positions[v] = position;
    for (size_t s = 0; s < expected_samples; ++s) {
      long long left, right;
      if (!pca_diploid_alleles(calls[s], &left, &right)) return false;
      in->set((v * expected_samples + s) * 2, left);
      in->set((v * expected_samples + s) * 2 + 1, right);
    }
  }
  return true;
}

// Vec<VariantInput> (lib.rs:834-873) -> compute_chromosome_pca's view of it (pca.rs:68-91): a site is complete when every genotype is
// Some with at least two alleles
// false = the sample-count error of pca.rs:69-77 in `*parse_error`
bool pca_input_from_variants(const py::handle& variants, size_t expected_samples, PcaInput* in, string* parse_error) {
  if (py::isinstance<py::str>(variants)) raise(PyExc_TypeError, "Can't extract `str` to `Vec`");
  vector<ParsedVariant> parsed;
  for (py::handle v : py::reinterpret_borrow<py::object>(variants)) parsed.push_back(parse_variant(v));
  in->variant_rule = true;
  in->resize(parsed.size(), expected_samples);
  in->positions.resize(parsed.size());
  for (size_t v = 0; v < parsed.size(); ++v) {
    const ParsedVariant& pv = parsed[v];
    if (pv.len.size() != expected_samples) {
      *parse_error = "variant " + std::to_string(v) + " contains " + std::to_string(pv.len.size()) + " samples but " + std::to_string(expected_samples) +
                     " names were provided";
      return false;
    }
    in->positions[v] = pv.position;
    for (size_t s = 0; s < expected_samples; ++s) {
      const size_t idx = (v * expected_samples + s) * 2;
      if (pv.len[s] < 2) { in->set(idx, -1); in->set(idx + 1, -1); continue; }
      in->set(idx, pv.alleles[pv.off[s]]);
      in->set(idx + 1, pv.alleles[pv.off[s] + 1]);
    }
  }
  return true;
}

void pca_validate(const vector<string>& sample_names, size_t n_components) {  // first of all: lib.rs:2053-2062
  if (sample_names.empty()) value_error("sample_names must contain at least one sample");
  if (n_components == 0) value_error("n_components must be greater than or equal to 1");
}

// labels, TSV text and the file writer: pca_host.hpp
vector<string> pca_labels(const vector<string>& sample_names) { return fmpca::labels(sample_names); }
string pca_tsv_text(const vector<string>& labels, const double* coordinates, size_t rows, size_t components) {
  return fmpca::tsv_text(labels, coordinates, rows, components);
}
bool pca_write_file(const std::filesystem::path& path, const string& text, string* error) { return fmpca::write_file(path, text, error); }

py::object chromosome_pca(const py::object& variants, const vector<string>& sample_names, size_t n_components) {
  pca_validate(sample_names, n_components);
  PcaInput in;
  bool dense = false;
  if (py::isinstance<py::dict>(variants) && py::reinterpret_borrow<py::dict>(variants).contains("genotypes")) {
    pca_input_from_mapping(py::reinterpret_borrow<py::dict>(variants), sample_names.size(), &in);
    dense = true;
  } else if (PyList_Check(variants.ptr())) {
    dense = pca_input_from_list(py::reinterpret_borrow<py::list>(variants), sample_names.size(), &in);
  }
  PcaOutput out;
  string parse_error;
  if (!dense) {
    in = PcaInput();
    if (!pca_input_from_variants(variants, sample_names.size(), &in, &parse_error)) vcf_error("Parse", parse_error);
  }
  if (!pca_compute(in, n_components, &out, &parse_error)) vcf_error("Parse", parse_error);
  ChromosomePcaResult result;
  result.haplotype_labels = pca_labels(sample_names);
  result.coordinates = py::array_t<double>({(py::ssize_t)out.haplotypes, (py::ssize_t)out.components});
  if (!out.coordinates.empty()) memcpy(result.coordinates.mutable_data(), out.coordinates.data(), out.coordinates.size() * sizeof(double));
  result.positions = py::array_t<int64_t>((py::ssize_t)out.positions.size());
  if (!out.positions.empty()) memcpy(result.positions.mutable_data(), out.positions.data(), out.positions.size() * sizeof(int64_t));
  return py::cast(std::move(result));
}

void chromosome_pca_to_file(const py::object& variants, const vector<string>& sample_names, const string& chromosome, const string& output_dir,
                            size_t n_components) {
  pca_validate(sample_names, n_components);
  PcaInput in;
  PcaOutput out;
  string error;
  if (!pca_input_from_variants(variants, sample_names.size(), &in, &error)) vcf_error("Parse", error);  // Vec<VariantInput> only, lib.rs:2099
  if (!pca_compute(in, n_components, &out, &error)) vcf_error("Parse", error);
  const string text = pca_tsv_text(pca_labels(sample_names), out.coordinates.data(), out.haplotypes, out.components);
  if (!pca_write_file(std::filesystem::path(output_dir) / ("pca_chr_" + chromosome + ".tsv"), text, &error)) vcf_error("Io", error);
}

// run_chromosome_pca_analysis, pca.rs:896-981: chromosomes with fewer than two variants are skipped, one that fails is passed over,
// none succeeding is the error
void per_chromosome_pca(const py::object& variants_by_chromosome, const vector<string>& sample_names, const string& output_dir, size_t n_components) {
  pca_validate(sample_names, n_components);
  if (!py::isinstance<py::dict>(variants_by_chromosome)) value_error("variants_by_chromosome must be a dict mapping chromosome -> sequence of variants");
  vector<std::pair<string, PcaInput>> inputs;
  for (auto item : py::reinterpret_borrow<py::dict>(variants_by_chromosome)) {
    const string chromosome = py::cast<string>(item.first);
    PcaInput in;
    string error;
    // a sample-count mismatch is that chromosome's failure (passed over), anything else an extraction error of the whole call
    if (!pca_input_from_variants(item.second, sample_names.size(), &in, &error)) in.variants = 0;
    inputs.emplace_back(chromosome, std::move(in));
  }
  std::error_code ec;
  std::filesystem::create_directories(output_dir, ec);
  if (ec) vcf_error("Io", ec.message() + ": " + output_dir);
  size_t successful = 0;
  for (auto& [chromosome, in] : inputs) {
    if (in.variants < 2) continue;
    PcaOutput out;
    string error;
    if (!pca_compute(in, n_components, &out, &error)) continue;
    const string text = pca_tsv_text(pca_labels(sample_names), out.coordinates.data(), out.haplotypes, out.components);
    if (pca_write_file(std::filesystem::path(output_dir) / ("pca_chr_" + chromosome + ".tsv"), text, &error)) ++successful;
  }
  if (successful == 0) vcf_error("Parse", "Failed to compute PCA for any chromosome");
}

// combine_chromosome_pca_results, pca.rs:985-1103 - the one piece global_pca lacks besides per_chromosome_pca: every pca_chr_*.tsv
// of results_dir, in file-name order, into one table with a Chromosome column after the haplotype
void combine_pca_results(const string& results_dir, const string& output_file) {
  namespace fs = std::filesystem;
  std::error_code ec;
  vector<fs::path> files;
  fs::directory_iterator it(results_dir, ec);
  if (ec) vcf_error("Io", ec.message() + ": " + results_dir);
  for (const fs::directory_entry& entry : it)
    if (entry.is_regular_file(ec) && entry.path().string().find("pca_chr_") != string::npos) files.push_back(entry.path());
  if (files.empty()) vcf_error("Parse", "No chromosome PCA result files found");
  std::sort(files.begin(), files.end(), [](const fs::path& a, const fs::path& b) { return a.filename().string() < b.filename().string(); });
  auto read_lines = [](const fs::path& p, vector<string>* lines) {  // str::lines: split at \n, a trailing \r dropped
    std::ifstream f(p, std::ios::binary);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    const string text = ss.str();
    size_t begin = 0;
    while (begin < text.size()) {
      size_t end = text.find('\n', begin);
      if (end == string::npos) end = text.size();
      string line = text.substr(begin, end - begin);
      if (!line.empty() && line.back() == '\r') line.pop_back();
      lines->push_back(std::move(line));
      begin = end + 1;
    }
    return true;
  };
  vector<string> first;
  if (!read_lines(files[0], &first)) vcf_error("Io", string(strerror(errno)) + ": " + files[0].string());
  if (first.empty()) vcf_error("Parse", "Empty PCA result file");
  const size_t n_components = (size_t)std::count(first[0].begin(), first[0].end(), '\t');  // columns minus the Haplotype one
  string text = "Haplotype\tChromosome";
  for (size_t k = 0; k < n_components; ++k) text += "\tPC" + std::to_string(k + 1);
  text += "\n";
  for (const fs::path& p : files) {
    const string name = p.filename().string();
    string chromosome = name;
    if (name.size() >= 12 && name.compare(0, 8, "pca_chr_") == 0 && name.compare(name.size() - 4, 4, ".tsv") == 0) chromosome = name.substr(8, name.size() - 12);
    vector<string> lines;
    if (!read_lines(p, &lines)) continue;
    for (size_t i = 1; i < lines.size(); ++i) {
      const size_t tab = lines[i].find('\t');
      if (tab == string::npos) continue;  // fewer than two fields
      text += lines[i].substr(0, tab) + "\t" + chromosome + lines[i].substr(tab) + "\n";
    }
  }
  string error;
  if (!pca_write_file(output_file, text, &error)) vcf_error("Io", error);
}

// the host eigen solver of the library, for tests: (eigenvalues ascending, eigenvectors as columns)
py::tuple pca_eigen_host(py::array_t<double, py::array::c_style | py::array::forcecast> matrix) {
  if (matrix.ndim() != 2 || matrix.shape(0) != matrix.shape(1) || matrix.shape(0) == 0) value_error("matrix must be square and non-empty");
  const size_t n = (size_t)matrix.shape(0);
  py::array_t<double> vectors({(py::ssize_t)n, (py::ssize_t)n});
  memcpy(vectors.mutable_data(), matrix.data(), n * n * sizeof(double));
  py::array_t<double> values((py::ssize_t)n);
  int rc;
  { py::gil_scoped_release nogil; rc = fmh_pca_eigen_host(vectors.mutable_data(), n, values.mutable_data()); }
  fmh_check(rc);
  return py::make_tuple(values, vectors);
}

void bind_pca(py::module_& m) {
  py::class_<ChromosomePcaResult>(m, "ChromosomePcaResult")
      .def_readonly("haplotype_labels", &ChromosomePcaResult::haplotype_labels)
      .def_readonly("coordinates", &ChromosomePcaResult::coordinates)
      .def_readonly("positions", &ChromosomePcaResult::positions)
      .def("__repr__", &ChromosomePcaResult::repr);
  m.def("chromosome_pca", &chromosome_pca, py::arg("variants"), py::arg("sample_names"), py::arg("n_components") = 10);
  m.def("chromosome_pca_to_file", &chromosome_pca_to_file, py::arg("variants"), py::arg("sample_names"), py::arg("chromosome"), py::arg("output_dir"),
        py::arg("n_components") = 10);
  m.def("per_chromosome_pca", &per_chromosome_pca, py::arg("variants_by_chromosome"), py::arg("sample_names"), py::arg("output_dir"),
        py::arg("n_components") = 10);
  m.def("_combine_pca_results", &combine_pca_results, py::arg("results_dir"), py::arg("output_file"));
  m.def("_pca_tsv_text", [](const vector<string>& labels, py::array_t<double, py::array::c_style | py::array::forcecast> coordinates) {
    if (coordinates.ndim() != 2) value_error("coordinates must be two-dimensional");
    return pca_tsv_text(labels, coordinates.data(), (size_t)coordinates.shape(0), (size_t)coordinates.shape(1));
  }, py::arg("labels"), py::arg("coordinates"));
  m.def("_pca_eigen_host", &pca_eigen_host, py::arg("matrix"));
}
