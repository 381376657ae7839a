// pymodule_rows.inc — what the device statistics' Python entry points share (included inside pymodule_stats.inc's namespace, before the
// per-statistic files): the rows a call runs over, the samples and haplotypes in play, the `samples` and `sites` arguments, and the small
// pieces of the chunk loops and from_sums constructors.  The pybind11 twin of stat_call.hpp: one wording of every rule, the statistic's
// noun passed in where the messages differ.  The steps stay separate (samples, then rows, then the upload) because the ORDER in which an
// entry point refuses its arguments is part of its surface and differs between the families; each entry point composes them in its order.

// a status of the library whose INVALID is the caller's arguments: a ValueError with the library's message; anything else is fmh_check's
void fmh_check_args(int status) {
  if (status == FMH_ERR_INVALID) value_error(fmh_last_error());
  fmh_check(status);
}

template <class T> py::array_t<T> array_of(const vector<T>& v) {
  py::array_t<T> out((py::ssize_t)v.size());
  if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(T));
  return out;
}

template <class T> vector<T> vector_arg(const py::object& obj, const char* name, size_t expect, bool check) {
  auto arr = py::array_t<T, py::array::c_style | py::array::forcecast>::ensure(obj);
  if (!arr || arr.ndim() != 1) value_error(string(name) + " must be a one-dimensional integer array");
  if (check && (size_t)arr.shape(0) != expect) value_error(string(name) + " has " + std::to_string(arr.shape(0)) + " entries, expected " + std::to_string(expect));
  return vector<T>(arr.data(), arr.data() + arr.shape(0));
}

// an i64 table argument of a from_sums constructor, flattened; it holds `expect` integers (kAnySize: however many) or "<name> must <what>"
constexpr size_t kAnySize = (size_t)-1;
vector<long long> i64_table_arg(const py::object& obj, const char* name, size_t expect, const string& what) {
  auto arr = py::array_t<long long, py::array::c_style | py::array::forcecast>::ensure(obj);
  if (!arr || (expect != kAnySize && (size_t)arr.size() != expect)) value_error(string(name) + " must " + what);
  return vector<long long>(arr.data(), arr.data() + arr.size());
}

// ---- rows ---------------------------------------------------------------------------------------------------------------------------------
// rows of a resident matrix and the columns in play: (matrix, first row, rows, column mask); rows == 0 = nothing to do
struct ResidentRows {
  shared_ptr<DevMatrix> dm;
  size_t r0 = 0, rc = 0;
  vector<uint8_t> mask;
};

optional<Region> region_arg(const py::object& region) { return region.is_none() ? std::nullopt : optional<Region>(build_region(region)); }

size_t variant_count(const Population& pop) { return pop.dense ? (size_t)pop.dense->variants : (size_t)pop.store->S; }

// The rows a call runs over: how many, their positions, and where they live.  Nothing is uploaded until resident() is asked: the windowed
// statistics ask only when some window holds a row.  `store` is the region's subset when a region was given; it lives as long as this does.
struct RowsInPlay {
  size_t count = 0;               // 0 = nothing to do: store and dense are empty
  shared_ptr<const Store> store;  // holds the rows' positions, and the rows themselves unless `dense` does
  shared_ptr<Dense> dense;        // a from_numpy Population's matrix

  // the rows' positions are the first `count` entries
  const vector<int64_t>& positions() const {
    static const vector<int64_t> none;
    return store ? store->positions : none;
  }
  vector<int64_t> positions_copy() const { return vector<int64_t>(positions().begin(), positions().begin() + (std::ptrdiff_t)count); }
  ResidentRows resident(vector<uint8_t> mask = {}) const {
    ResidentRows out;
    if (count == 0) return out;
    out.mask = std::move(mask);
    if (dense) {
      out.dm = dense->device_matrix();
      out.rc = out.dm->variants;
      return out;
    }
    auto [dm, r0, rc] = store->device_rows();
    out.dm = dm; out.r0 = r0; out.rc = rc;
    return out;
  }
};

// every variant of a store, or those inside a region
RowsInPlay rows_in_play(const shared_ptr<const Store>& store, const optional<Region>& region) {
  RowsInPlay out;
  if (store->S == 0) return out;
  out.store = store;
  if (region) {
    const vector<int64_t> rows = region_len(*region) > 0 ? region_rows(*store, region->start, region->end) : vector<int64_t>();
    out.store = rows.empty() ? nullptr : store_subset(store, rows);
  }
  if (out.store) out.count = (size_t)out.store->S;
  return out;
}
// the same with `region` as it came from Python, read only when there is a variant: the cohort statistics' and LD's order (the haplotype
// windows parse it before they look at the variants, with region_arg)
RowsInPlay rows_in_play(const shared_ptr<const Store>& store, const py::object& region) {
  return rows_in_play(store, store->S == 0 ? std::nullopt : region_arg(region));
}
// a Population's variants: the dense matrix of from_numpy, else the variant store's
RowsInPlay rows_in_play(const Population& pop) {
  RowsInPlay out;
  out.count = std::min(variant_count(pop), pop.store->positions.size());
  if (out.count == 0) return out;
  out.store = pop.store;
  out.dense = pop.dense;
  return out;
}

// ---- samples and haplotypes -----------------------------------------------------------------------------------------------------------------
// the cohort statistics read genotypes: "<noun> diploid genotypes (ploidy 2), got ploidy P" once there is a variant to have a ploidy
void diploid_only(int64_t ploidy, size_t count, const char* noun) {
  if (count != 0 && ploidy != 2) value_error(string(noun) + " diploid genotypes (ploidy 2), got ploidy " + std::to_string(ploidy));
}
void diploid_only(const Population& pop, const char* noun) { diploid_only(pop.dense ? pop.dense->ploidy : pop.store->P, variant_count(pop), noun); }

// the samples BOTH of whose haplotypes belong to the population, ascending
vector<uint32_t> population_samples(const Population& pop) {
  const int64_t limit = pop.dense ? pop.dense->samples : pop.store->first_sample_count();
  vector<uint8_t> sides((size_t)std::max<int64_t>(limit, 0), 0);
  for (auto& h : pop.haplotypes)
    if (h.first >= 0 && h.first < limit) sides[(size_t)h.first] |= h.second == kLeft ? 1 : 2;
  vector<uint32_t> list;
  for (size_t s = 0; s < sides.size(); ++s)
    if (sides[s] == 3) list.push_back((uint32_t)s);
  return list;
}

// a Population's own haplotypes as a column mask of its resident matrix
vector<uint8_t> population_mask(const Population& pop) {
  return pop.dense ? pop.dense->mask_for(pop.haplotypes) : pop.store->mask_for(pop.haplotypes, pop.store->first_sample_count());
}

// a Population's own haplotypes over its resident matrix
ResidentRows resident_rows_of(const Population& pop) { return rows_in_play(pop).resident(population_mask(pop)); }

// The haplotype statistics' columns and sample size, the second of their two steps: the entry point has refused an empty list already
// (`sample_size(haps, nullptr)`: hap_sample_size or sfs_sample_size, whose words differ) and the variants are known now.  Without a variant
// there are no columns to look the haplotypes up in and the size is len(haplotypes); else membership is taken from the FIRST variant's
// sample count and `sample_size(haps, &mask)` refuses what it has to.
struct HapColumns {
  vector<uint8_t> mask;
  size_t n = 0;
};
using HapSampleSize = size_t (*)(const vector<Hap>&, const vector<uint8_t>*);
HapColumns hap_columns(const Store& store, const vector<Hap>& haps, HapSampleSize sample_size) {
  HapColumns out;
  out.n = haps.size();
  if (store.S == 0) return out;
  out.mask = store.mask_for(haps, store.first_sample_count());
  out.n = sample_size(haps, &out.mask);
  return out;
}
HapColumns hap_columns(const Population& pop, HapSampleSize sample_size) {
  HapColumns out;
  out.n = pop.haplotypes.size();
  if (variant_count(pop) == 0) return out;
  out.mask = population_mask(pop);
  out.n = sample_size(pop.haplotypes, &out.mask);
  return out;
}

// the `sites` argument: None, or a boolean array with one entry per row in play
vector<uint8_t> site_mask_arg(const py::object& sites, size_t rows, bool* given) {
  *given = !sites.is_none();
  vector<uint8_t> keep;
  if (!*given) return keep;
  auto arr = py::array_t<bool, py::array::c_style | py::array::forcecast>::ensure(sites);
  if (!arr || arr.ndim() != 1) value_error("sites must be a one-dimensional boolean array");
  if ((size_t)arr.shape(0) != rows) value_error("sites has " + std::to_string(arr.shape(0)) + " entries for " + std::to_string(rows) + " rows");
  keep.resize(rows);
  const bool* p = arr.data();
  for (size_t i = 0; i < rows; ++i) keep[i] = p[i] ? 1 : 0;
  return keep;
}

// the `samples` argument: None = every sample, else strictly ascending sample numbers below `limit`
vector<uint32_t> sample_list_arg(const py::object& samples, int64_t limit) {
  vector<uint32_t> out;
  if (samples.is_none()) {
    for (int64_t s = 0; s < limit; ++s) out.push_back((uint32_t)s);
    return out;
  }
  for (const py::handle& item : py::iter(samples)) {
    if (!is_intlike(item)) raise(PyExc_TypeError, "samples must be integers");
    const int64_t s = to_i64(item);
    if (s < 0 || s >= limit) value_error("sample " + std::to_string(s) + " is outside the variants' " + std::to_string(limit) + " samples");
    if (!out.empty() && (int64_t)out.back() >= s) value_error("samples must be strictly ascending");
    out.push_back((uint32_t)s);
  }
  return out;
}

// ---- row chunks ---------------------------------------------------------------------------------------------------------------------------
// rows per chunk of `rows` rows at `row_bytes` each under the byte budget the option names: at least one
size_t chunk_rows_under(const char* budget_option, size_t rows, size_t row_bytes) {
  long long budget = 0;
  fmh_check(fmh_get_option(budget_option, &budget));
  return std::min(rows, std::max<size_t>(1, (size_t)std::max<long long>(budget, 0) / row_bytes));
}

// the site tracks of a chunk (hom-ref, het and hom-alt counts per row): what fmh_genotype_counts writes on the device, and a host copy
struct ChunkTracks {
  size_t rows;
  DevBuf buf;
  fmh_genotype_site_out site;
  vector<uint32_t> host;
  ChunkTracks(int device, size_t chunk_rows)
      : rows(chunk_rows), buf(device, 3 * chunk_rows * sizeof(uint32_t)),
        site{(uint32_t*)buf.p, (uint32_t*)buf.p + chunk_rows, (uint32_t*)buf.p + 2 * chunk_rows}, host(3 * chunk_rows) {}
  int download() { return fmh_copy_to_host(buf.device, host.data(), buf.p, 3 * rows * sizeof(uint32_t), nullptr); }  // a library status
  const uint32_t* ref() const { return host.data(); }
  const uint32_t* het() const { return host.data() + rows; }
  const uint32_t* alt() const { return host.data() + 2 * rows; }
};
