// pymodule_admix.inc — ferromic.admixture, Population.admixture and the Admixture result (included inside pymodule_stats.inc's namespace, after
// pymodule_rows.inc whose rows and sample rules it uses).  An addition to the reference's surface: it has no ancestry model; the definition is
// include/ferromic_hip.h's (fmh_admix_create, fmh_admix_step, fmh_admix_start, fmh_admix_accelerate).  The EM steps run on the device from the
// handle's resident genotype image; the extrapolation of an accelerated cycle is host arithmetic of the library between them; the GIL is
// released around the fit.

struct Admixture {
  vector<uint32_t> samples;
  vector<int64_t> sites, positions;  // the kept rows as indices into the rows in play, and their positions
  size_t k = 0;
  vector<double> q, frequencies;     // [n][K], [kept rows][K] (NaN on rows that are not usable)
  double log_likelihood = std::numeric_limits<double>::quiet_NaN();
  vector<double> trace;              // one l per EM step taken (the l of that step's input)
  uint64_t steps = 0, cycles = 0, accepted = 0, n_usable = 0;
  bool converged = false;
  vector<uint8_t> usable;
  vector<uint32_t> called, allele_count;
  vector<uint64_t> sample_sites;

  py::array_t<double> table(const vector<double>& v, size_t rows) const {
    py::array_t<double> out(std::vector<py::ssize_t>{(py::ssize_t)rows, (py::ssize_t)k});
    if (!v.empty()) memcpy(out.mutable_data(), v.data(), v.size() * sizeof(double));
    return out;
  }
  string repr() const {
    return "Admixture(samples=" + std::to_string(samples.size()) + ", sites=" + std::to_string(sites.size()) + ", usable=" + std::to_string(n_usable) +
           ", k=" + std::to_string(k) + ", steps=" + std::to_string(steps) + ")";
  }
};

struct AdmixHandle {
  fmh_admix* h = nullptr;
  AdmixHandle() = default;
  AdmixHandle(const AdmixHandle&) = delete;
  ~AdmixHandle() { if (h) fmh_admix_destroy(h); }
};

// what the arguments say before any device is used
struct AdmixArgsIn {
  size_t K = 0;
  bool accelerate = true, projection = false, has_init = false, has_init_f = false;
  double tol = 0.0;
  uint64_t max_steps = 0, seed = 0;
  F64Array init_q, init_f, fixed_f;
};

AdmixArgsIn admix_args(int64_t k, const py::object& init, const py::object& seed, bool accelerate, double tol, int64_t max_steps, const py::object& frequencies,
                       size_t n) {
  AdmixArgsIn in;
  if (k < 1 || k > FMH_ADMIX_MAX_K) value_error("k must be 1 to " + std::to_string(FMH_ADMIX_MAX_K) + ", got " + std::to_string(k));
  if (n == 0) value_error("at least one sample is required for admixture");
  if (!(tol >= 0.0) || !std::isfinite(tol)) value_error("tol must be a finite number that is not negative");
  if (max_steps < 0) value_error("max_steps must not be negative");
  if (!is_intlike(seed) || to_i64(seed) < 0) value_error("seed must be an integer that is not negative");
  in.K = (size_t)k;
  in.accelerate = accelerate;
  in.tol = tol;
  in.max_steps = (uint64_t)max_steps;
  in.seed = (uint64_t)to_i64(seed);
  const size_t K = in.K;
  if (!frequencies.is_none()) {
    in.fixed_f = F64Array::ensure(frequencies);
    if (!in.fixed_f || in.fixed_f.ndim() != 2 || (size_t)in.fixed_f.shape(1) != K) value_error("frequencies must be a numeric array [rows][k]");
    in.projection = true;
  }
  if (!init.is_none()) {
    if (!py::isinstance<py::tuple>(init) && !py::isinstance<py::list>(init)) value_error("init must be (Q [n][k], F [rows][k])");
    const py::sequence pair = init.cast<py::sequence>();
    if (pair.size() != 2) value_error("init must be (Q [n][k], F [rows][k])");
    in.init_q = F64Array::ensure(pair[0]);
    if (!in.init_q || in.init_q.ndim() != 2 || (size_t)in.init_q.shape(0) != n || (size_t)in.init_q.shape(1) != K)
      value_error("init's Q must be [n][k] with one row per selected sample (" + std::to_string(n) + ")");
    for (py::ssize_t e = 0; e < in.init_q.size(); ++e) {
      const double v = in.init_q.data()[e];
      if (!(v > 0.0) || !(v <= 1.0)) value_error("init's Q holds a value outside (0, 1]");
    }
    if (py::object(pair[1]).is_none()) {
      if (!in.projection) value_error("init's F is None: that is taken only with frequencies=");
    } else {
      if (in.projection) value_error("init's F and frequencies= are both given");
      in.init_f = F64Array::ensure(pair[1]);
      if (!in.init_f || in.init_f.ndim() != 2 || (size_t)in.init_f.shape(1) != K) value_error("init's F must be a numeric array [rows][k]");
      in.has_init_f = true;
    }
    in.has_init = true;
  }
  return in;
}

// F [kept][K] as the caller gave it -> [m][K] over the usable rows, each value checked
vector<double> admix_compact_f(const F64Array& f, const vector<uint8_t>& usable, size_t kept, size_t K, const char* name) {
  if ((size_t)f.shape(0) != kept) value_error(string(name) + " has " + std::to_string(f.shape(0)) + " rows, expected one per kept row (" + std::to_string(kept) + ")");
  vector<double> out;
  for (size_t r = 0; r < kept; ++r) {
    if (!usable[r]) continue;
    for (size_t c = 0; c < K; ++c) {
      const double v = f.data()[r * K + c];
      if (!(v > 0.0) || !(v < 1.0)) value_error(string(name) + " holds a value outside (0, 1) on usable row " + std::to_string(r));
      out.push_back(v);
    }
  }
  return out;
}

Admixture admixture_over_rows(const RowsInPlay& in_play, vector<uint32_t> samples, const py::object& sites, const AdmixArgsIn& in) {
  const ResidentRows rows = in_play.resident();
  const shared_ptr<DevMatrix>& dm = rows.dm;
  const size_t r0 = rows.r0, rc = rows.rc;
  Admixture out;
  out.samples = std::move(samples);
  out.k = in.K;
  const size_t n = out.samples.size(), K = in.K;
  bool masked = false;
  const vector<uint8_t> keep = site_mask_arg(sites, rc, &masked);
  for (size_t i = 0; i < rc; ++i)
    if (!masked || keep[i]) out.sites.push_back((int64_t)i);
  const size_t kept = out.sites.size();
  const vector<int64_t>& pos = in_play.positions();
  for (int64_t r : out.sites)
    if ((size_t)r < pos.size()) out.positions.push_back(pos[(size_t)r]);
  out.usable.assign(kept, 0);
  out.called.assign(kept, 0);
  out.allele_count.assign(kept, 0);
  out.sample_sites.assign(n, 0);
  out.frequencies.assign(kept * K, std::numeric_limits<double>::quiet_NaN());
  out.q.assign(n * K, 0.0);

  AdmixHandle handle;
  const int device = dm ? dm->device : current_device();
  size_t m = 0;
  if (dm && rc != 0) {
    int status;
    fmh_admix_info_out info{};
    {
      py::gil_scoped_release nogil;
      status = fmh_admix_create(dm->h, out.samples.data(), n, r0, rc, masked ? keep.data() : nullptr, &handle.h, nullptr);
      if (status == FMH_OK) status = fmh_admix_info(handle.h, &info);
    }
    fmh_check(status);
    m = (size_t)info.usable_rows;
    std::copy(info.h_usable, info.h_usable + kept, out.usable.begin());
    std::copy(info.h_called, info.h_called + kept, out.called.begin());
    std::copy(info.h_allele_count, info.h_allele_count + kept, out.allele_count.begin());
    std::copy(info.h_sample_sites, info.h_sample_sites + n, out.sample_sites.begin());
  }
  out.n_usable = m;

  // ---- the start ----
  vector<uint32_t> cu, au;
  for (size_t r = 0; r < kept; ++r)
    if (out.usable[r]) { cu.push_back(out.called[r]); au.push_back(out.allele_count[r]); }
  vector<double> q(n * K), f(m * K);
  fmh_check(fmh_admix_start(cu.data(), au.data(), m, n, K, in.seed, q.data(), f.data()));
  if (in.has_init) q.assign(in.init_q.data(), in.init_q.data() + n * K);
  if (in.has_init_f) f = admix_compact_f(in.init_f, out.usable, kept, K, "init's F");
  if (in.projection) f = admix_compact_f(in.fixed_f, out.usable, kept, K, "frequencies");

  auto finish = [&]() {
    out.q = q;
    for (size_t r = 0, j = 0; r < kept; ++r) {
      if (!out.usable[r]) continue;
      for (size_t c = 0; c < K; ++c) out.frequencies[r * K + c] = f[j * K + c];
      ++j;
    }
  };
  if (m == 0) {
    out.log_likelihood = 0.0;
    finish();
    return out;
  }

  // ---- the fit: device steps on ping-pong buffers, the extrapolation on the host ----
  const size_t qb = n * K * sizeof(double), fb = m * K * sizeof(double);
  const uint32_t flags = FMH_ADMIX_UPDATE_Q | (in.projection ? 0u : FMH_ADMIX_UPDATE_F);
  const size_t mf = in.projection ? 0 : m;  // F takes part in the extrapolation unless it is fixed
  DevBuf dq0(device, qb), dq1(device, qb), dq2(device, qb), dq3(device, qb), df0(device, fb), df1(device, fb), df2(device, fb), df3(device, fb);
  int status = FMH_OK;
  {
    py::gil_scoped_release nogil;
    auto up = [&](DevBuf& dq, DevBuf& df, const vector<double>& hq, const vector<double>& hf) {
      if (status == FMH_OK) status = fmh_copy_to_device(device, dq.p, hq.data(), qb, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_device(device, df.p, hf.data(), fb, nullptr);
    };
    auto down = [&](const DevBuf& dq, const DevBuf& df, vector<double>& hq, vector<double>& hf) {
      if (status == FMH_OK) status = fmh_copy_to_host(device, hq.data(), dq.p, qb, nullptr);
      if (status == FMH_OK) status = fmh_copy_to_host(device, hf.data(), df.p, fb, nullptr);
    };
    auto step = [&](const DevBuf& sq, const DevBuf& sf, DevBuf& tq, DevBuf& tf, uint32_t fl, double* ll) {
      if (status == FMH_OK)
        status = fmh_admix_step(handle.h, K, (const double*)sq.p, (const double*)sf.p, (double*)tq.p, (double*)tf.p, ll, fl, nullptr);
      if (status == FMH_OK && ll) out.trace.push_back(*ll);
    };
    DevBuf *cq = &dq0, *cf = &df0;  // where the current state lives
    up(dq0, df0, q, f);
    double previous = 0.0;
    bool have_previous = false;
    if (!in.accelerate) {
      DevBuf *oq = &dq1, *of = &df1;
      while (status == FMH_OK && out.steps < in.max_steps) {
        double ll = 0.0;
        step(*cq, *cf, *oq, *of, flags, &ll);
        std::swap(cq, oq);
        std::swap(cf, of);
        ++out.steps;
        const bool done = have_previous && in.tol > 0.0 && ll - previous < in.tol;
        previous = ll;
        have_previous = true;
        if (done) { out.converged = true; break; }
      }
      down(*cq, *cf, q, f);
    } else {
      vector<double> q1(n * K), f1(m * K), q2(n * K), f2(m * K), qa(n * K), fa(m * K);
      while (status == FMH_OK && out.steps + 3 <= in.max_steps) {
        // theta0 = (q, f) lives in dq0 / df0
        double l0 = 0.0, l1 = 0.0, la = 0.0, alpha = 0.0;
        step(dq0, df0, dq1, df1, flags, &l0);
        step(dq1, df1, dq2, df2, flags, &l1);
        out.steps += 2;
        ++out.cycles;
        down(dq1, df1, q1, f1);
        down(dq2, df2, q2, f2);
        if (status != FMH_OK) break;
        const bool done = have_previous && in.tol > 0.0 && l0 - previous < in.tol;
        previous = l0;
        have_previous = true;
        status = fmh_admix_accelerate(q.data(), f.data(), q1.data(), f1.data(), q2.data(), f2.data(), n, mf, K, qa.data(), fa.data(), &alpha);
        if (status != FMH_OK) break;
        bool kept_it = false;
        if (alpha != 0.0 && !done) {
          if (mf == 0) fa = f;
          up(dq3, df3, qa, fa);
          step(dq3, df3, dq0, df0, flags, &la);
          ++out.steps;
          kept_it = status == FMH_OK && std::isfinite(la) && la >= l1;
          if (kept_it) { down(dq0, df0, q, f); ++out.accepted; }
        }
        if (!kept_it) {
          q = q2;
          f = f2;
          up(dq0, df0, q, f);
        }
        if (done) { out.converged = true; break; }
      }
      cq = &dq0;
      cf = &df0;
    }
    // l of the state that is returned: one pass that updates nothing
    double ll = 0.0;
    if (status == FMH_OK) status = fmh_admix_step(handle.h, K, (const double*)cq->p, (const double*)cf->p, (double*)dq3.p, (double*)df3.p, &ll, 0u, nullptr);
    out.log_likelihood = ll;
  }
  fmh_check(status);
  finish();
  return out;
}

Admixture admixture(const py::object& variants, int64_t k, const py::object& samples, const py::object& sites, const py::object& region, const py::object& init,
                    const py::object& seed, bool accelerate, double tol, int64_t max_steps, const py::object& frequencies) {
  auto store = store_from_python(variants);
  diploid_only(store->P, (size_t)store->S, "admixture takes");
  vector<uint32_t> list = sample_list_arg(samples, store->first_sample_count());
  const AdmixArgsIn in = admix_args(k, init, seed, accelerate, tol, max_steps, frequencies, list.size());
  return admixture_over_rows(rows_in_play(store, region), std::move(list), sites, in);
}

Admixture population_admixture(const Population& pop, int64_t k, const py::object& sites, const py::object& init, const py::object& seed, bool accelerate,
                               double tol, int64_t max_steps, const py::object& frequencies) {
  diploid_only(pop, "admixture takes");
  vector<uint32_t> list = population_samples(pop);
  const AdmixArgsIn in = admix_args(k, init, seed, accelerate, tol, max_steps, frequencies, list.size());
  return admixture_over_rows(rows_in_play(pop), std::move(list), sites, in);
}

// A result from a state that was computed before (no device): q [n][k], frequencies [rows][k]; every track is optional.
Admixture admixture_from_state(const py::object& q, const py::object& frequencies, const py::object& usable, const py::object& called,
                               const py::object& allele_count, const py::object& sample_sites, const py::object& samples, const py::object& sites,
                               const py::object& positions, double log_likelihood, const py::object& trace, uint64_t steps, uint64_t cycles, uint64_t accepted,
                               bool converged) {
  Admixture out;
  auto qv = F64Array::ensure(q), fv = F64Array::ensure(frequencies);
  if (!qv || qv.ndim() != 2 || qv.shape(0) < 1 || qv.shape(1) < 1) value_error("q must be a numeric array [n][k]");
  const size_t n = (size_t)qv.shape(0), K = (size_t)qv.shape(1);
  if (K > FMH_ADMIX_MAX_K) value_error("k must be 1 to " + std::to_string(FMH_ADMIX_MAX_K) + ", got " + std::to_string(K));
  if (!fv || fv.ndim() != 2 || (size_t)fv.shape(1) != K) value_error("frequencies must be a numeric array [rows][k] with q's k");
  const size_t rows = (size_t)fv.shape(0);
  out.k = K;
  out.q.assign(qv.data(), qv.data() + n * K);
  out.frequencies.assign(fv.data(), fv.data() + rows * K);
  if (!usable.is_none()) {
    auto uv = py::array_t<bool, py::array::c_style | py::array::forcecast>::ensure(usable);
    if (!uv || uv.ndim() != 1 || (size_t)uv.shape(0) != rows) value_error("usable must be a boolean array with one entry per row of frequencies");
    for (size_t r = 0; r < rows; ++r) out.usable.push_back(uv.data()[r] ? 1 : 0);
  } else {
    out.usable.assign(rows, 0);
    for (size_t r = 0; r < rows; ++r) out.usable[r] = out.frequencies[r * K] == out.frequencies[r * K] ? 1 : 0;
  }
  for (uint8_t u : out.usable) out.n_usable += u;
  if (!called.is_none()) out.called = vector_arg<uint32_t>(called, "called", rows, true);
  if (!allele_count.is_none()) out.allele_count = vector_arg<uint32_t>(allele_count, "allele_count", rows, true);
  if (!sample_sites.is_none()) out.sample_sites = vector_arg<uint64_t>(sample_sites, "sample_sites", n, true);
  if (!samples.is_none()) out.samples = vector_arg<uint32_t>(samples, "samples", n, true);
  else for (size_t i = 0; i < n; ++i) out.samples.push_back((uint32_t)i);
  if (!sites.is_none()) out.sites = vector_arg<int64_t>(sites, "sites", rows, true);
  else for (size_t r = 0; r < rows; ++r) out.sites.push_back((int64_t)r);
  if (!positions.is_none()) out.positions = vector_arg<int64_t>(positions, "positions", rows, true);
  if (!trace.is_none()) {
    auto tv = F64Array::ensure(trace);
    if (!tv || tv.ndim() != 1) value_error("trace must be a one-dimensional array");
    out.trace.assign(tv.data(), tv.data() + tv.size());
  }
  out.log_likelihood = log_likelihood;
  out.steps = steps;
  out.cycles = cycles;
  out.accepted = accepted;
  out.converged = converged;
  return out;
}

void bind_admix(py::module_& m, py::class_<Population, shared_ptr<Population>>& population) {
  py::class_<Admixture>(m, "Admixture")
      .def_static("from_state", &admixture_from_state, py::arg("q"), py::arg("frequencies"), py::arg("usable") = py::none(), py::arg("called") = py::none(),
                  py::arg("allele_count") = py::none(), py::arg("sample_sites") = py::none(), py::arg("samples") = py::none(), py::arg("sites") = py::none(),
                  py::arg("positions") = py::none(), py::arg("log_likelihood") = std::numeric_limits<double>::quiet_NaN(), py::arg("trace") = py::none(),
                  py::arg("steps") = 0, py::arg("cycles") = 0, py::arg("accepted") = 0, py::arg("converged") = false)
      .def_property_readonly("q", [](const Admixture& a) { return a.table(a.q, a.samples.size()); })
      .def_property_readonly("frequencies", [](const Admixture& a) { return a.table(a.frequencies, a.sites.size()); })
      .def_property_readonly("log_likelihood", [](const Admixture& a) { return a.log_likelihood; })
      .def_property_readonly("trace", [](const Admixture& a) { return array_of(a.trace); })
      .def_property_readonly("steps", [](const Admixture& a) { return a.steps; })
      .def_property_readonly("cycles", [](const Admixture& a) { return a.cycles; })
      .def_property_readonly("accepted", [](const Admixture& a) { return a.accepted; })
      .def_property_readonly("converged", [](const Admixture& a) { return a.converged; })
      .def_property_readonly("usable", [](const Admixture& a) {
        py::array_t<bool> out((py::ssize_t)a.usable.size());
        for (size_t i = 0; i < a.usable.size(); ++i) out.mutable_data()[i] = a.usable[i] != 0;
        return out;
      })
      .def_property_readonly("n_usable", [](const Admixture& a) { return a.n_usable; })
      .def_property_readonly("called", [](const Admixture& a) { return array_of(a.called); })
      .def_property_readonly("allele_count", [](const Admixture& a) { return array_of(a.allele_count); })
      .def_property_readonly("sample_sites", [](const Admixture& a) { return array_of(a.sample_sites); })
      .def_property_readonly("samples", [](const Admixture& a) {
        py::array_t<int64_t> out((py::ssize_t)a.samples.size());
        for (size_t i = 0; i < a.samples.size(); ++i) out.mutable_data()[i] = a.samples[i];
        return out;
      })
      .def_property_readonly("sites", [](const Admixture& a) { return array_of(a.sites); })
      .def_property_readonly("positions", [](const Admixture& a) { return array_of(a.positions); })
      .def_property_readonly("k", [](const Admixture& a) { return a.k; })
      .def("__repr__", &Admixture::repr);
  m.def("admixture", &admixture, py::arg("variants"), py::arg("k"), py::arg("samples") = py::none(), py::arg("sites") = py::none(), py::arg("region") = py::none(),
        py::arg("init") = py::none(), py::arg("seed") = 0, py::arg("accelerate") = true, py::arg("tol") = 1e-4, py::arg("max_steps") = 1500,
        py::arg("frequencies") = py::none());
  population.def("admixture", &population_admixture, py::arg("k"), py::arg("sites") = py::none(), py::arg("init") = py::none(), py::arg("seed") = 0,
                 py::arg("accelerate") = true, py::arg("tol") = 1e-4, py::arg("max_steps") = 1500, py::arg("frequencies") = py::none());
}
