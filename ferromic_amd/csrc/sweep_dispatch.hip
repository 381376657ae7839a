// sweep_dispatch.hip — every sweep's way to its kernel: plan (sweep_plan.hpp), kernel arguments, the route's launcher (sweep_*.hip),
// finalize.  enqueue_sweep serves the blocking statistic entry points of abi.hip (through run_sweep) and the sharded sweeps of comm.hip;
// fmh_sweep_window, fmh_sweep_tiled and fmh_sweep_prefix report what the plan of the next sweep says.
#include "abi_internal.hpp"
#include "sweep_plan.hpp"

using namespace fmh;
using namespace fmhi;

// one snapshot of the switches per plan (atomics; the environment is never read here)
static PlanOptions snapshot_plan_options() {
  const Options& o = options();
  PlanOptions s;
  s.layout_bytes = o.layout_bytes.load(std::memory_order_relaxed);
  s.mask_mode = o.mask_mode.load();
  s.defer_tiles = o.defer_tiles.load();
  s.packed_lpr = o.packed_lpr.load();
  s.packed_unroll = o.packed_unroll.load();
  s.packed_no_prefetch = o.packed_no_prefetch.load();
  s.counts_mfma = o.counts_mfma.load();
  s.unroll = o.unroll.load();
  s.flat = o.flat.load();
  s.wc_exact = o.wc_exact.load();
  s.column_window = o.column_window.load();
  s.tiled = o.tiled.load();
  s.prefix_counts = o.prefix_counts.load();
  return s;
}
static SweepPlan plan_of(const fmh_matrix* m, const fmh_groups* g, int mode, size_t row_count) {
  return plan_sweep(*m, *g, mode, row_count, snapshot_plan_options(), LdsFigures{device_lds_limit(m->device), device_lds_per_cu(m->device)});
}

int fmhi::wc_kernel_groups(const fmh_matrix* m, const fmh_groups* g) {
  if (!m || !g) return 0;
  return plan_wc_groups(*m, *g, snapshot_plan_options());
}
ColumnWindow fmhi::sweep_window(const fmh_matrix* m, const fmh_groups* g, int mode) { return plan_of(m, g, mode, 1).win; }

bool fmhi::wc_fused_lane_totals(const fmh_matrix* m, const fmh_groups* g) { return m && g && plan_wc_fused(*m, *g, device_lds_limit(m->device)); }
bool fmhi::summaries_single_sweep(const fmh_matrix* m, const fmh_groups* g) { return m && g && plan_summaries_single(*m, *g, device_lds_limit(m->device)); }

static int check_probe(const fmh_matrix* m, const fmh_groups* g) {
  if (!m || !g) return fail(FMH_ERR_INVALID, "matrix or groups is NULL");
  if (g->device != m->device || g->pitch != m->pitch || g->columns != m->columns)
    return fail(FMH_ERR_INVALID, "groups were built for a different matrix geometry");
  return FMH_OK;
}

extern "C" int fmh_sweep_tiled(const fmh_matrix* m, const fmh_groups* g, int mode, int* tiled, size_t* image_bytes) {
  FMH_TRY(check_probe(m, g));
  if (tiled) *tiled = plan_of(m, g, mode, 1).tiled ? 1 : 0;
  if (image_bytes) *image_bytes = m->p0t ? m->p0t_bytes : 0;
  return FMH_OK;
}

extern "C" int fmh_sweep_prefix(const fmh_matrix* m, const fmh_groups* g, int mode, int* uses_table, uint32_t* vectors_read, size_t* table_bytes) {
  FMH_TRY(check_probe(m, g));
  const SweepPlan plan = plan_of(m, g, mode, 1);
  if (uses_table) *uses_table = plan.prefix ? 1 : 0;
  if (vectors_read) *vectors_read = plan.prefix ? plan.prefix_vecs : plan.win.count;
  if (table_bytes) *table_bytes = m->p0c ? m->p0c_bytes : 0;
  return FMH_OK;
}

extern "C" int fmh_sweep_window(const fmh_matrix* m, const fmh_groups* g, int mode, uint32_t* first_vec, uint32_t* n_vec, int* derived_group) {
  FMH_TRY(check_probe(m, g));
  const ColumnWindow w = sweep_window(m, g, mode);
  if (first_vec) *first_vec = w.first;
  if (n_vec) *n_vec = w.count;
  if (derived_group) *derived_group = w.derived;
  return FMH_OK;
}

// Validates, plans, fills the kernel arguments from the plan and enqueues sweep + finalize on `st`: the 128 regional
// accumulators land in b.out_f64 / b.out_u64 (device).  No synchronisation and no use of the shared workspace buffers, so
// callers with private buffers (the pipelined sharded sweeps of comm.hip) need no device lock.  `*launched` = false when
// the row range is empty (nothing was enqueued; the totals are all zero).
int fmhi::enqueue_sweep(const fmh_matrix* m, const fmh_groups* g, int mode, SweepArgs& a, hipStream_t st, const LaunchCtx& ctx,
                        const SweepBuffers& b, const double* harmonic, bool* launched) {
  *launched = false;
  FMH_TRY(check_probe(m, g));
  if (a.row_begin > m->variants || a.row_count > m->variants - a.row_begin)
    return fail(FMH_ERR_INVALID, "row range [%zu, +%zu) exceeds %zu variants", a.row_begin, a.row_count, m->variants);
  FMH_TRY(use_device(m->device));
  if (!m->p0 && !m->data) return fail(FMH_ERR_INVALID, "matrix holds neither a byte nor a packed image");
  const SweepPlan plan = plan_of(m, g, mode, a.row_count);
  const int P = plan.P;
  if (plan.packed) {
    a.mv.data = m->p0;
    a.mv.data1 = m->p1;
    a.mv.data2 = m->p2;
    a.mv.bits = m->pc;
    a.mv.row_hi = m->row_hi;
    a.mv.row_gap = m->row_gap;
    a.mv.pitch = m->plane_pitch;
    a.mv.bits_pitch = m->plane_pitch;
    a.mv.nvec = m->pvec;
  } else {
    a.mv.data = m->data;
    a.mv.data1 = nullptr;
    a.mv.data2 = nullptr;
    a.mv.bits = m->bits;
    a.mv.row_hi = nullptr;
    a.mv.row_gap = nullptr;
    a.mv.pitch = m->pitch;
    a.mv.bits_pitch = m->bits_pitch;
    a.mv.nvec = m->nvec;
  }
  a.mv.columns = m->columns;
  a.masks = g->masks;
  a.mask_pitch = g->mask_pitch;
  a.mask_bits = g->mask_bits;
  a.mask_flat = g->mask_flat;
  // the column window: plane 0 (row-major, or the tiled image: 1 KiB per vector and tile) and the bit masks advance to its first vector, the
  // row is as long as the window; pitch and columns stay the row's.  (The whole row and nothing derived: the launch is the one without a
  // window, byte for byte.)
  const ColumnWindow& win = plan.win;
  a.derived_group = -1;
  a.row_alt = nullptr;
  if (plan.tiled || plan.windowed) {
    a.mv.data = plan.tiled ? m->p0t + (size_t)win.first * 1024 : m->p0 + (size_t)win.first * 16;
    a.mv.nvec = win.count;
    a.mask_bits = g->mask_bits + (size_t)win.first * 8;  // one 16-bit word per 16 columns: eight per vector
    a.derived_group = win.derived;
    a.row_alt = win.derived >= 0 ? m->row_alt : nullptr;
  }
  // the table form: the whole image, the prefix counts and the counted groups' entries and edges; the masks are not read
  a.prefix = nullptr;
  if (plan.prefix) {
    a.mv.data = m->p0t;
    a.mv.nvec = plan.prefix_vecs;
    a.prefix = m->p0c;
    a.prefix_group[0] = plan.prefix_group[0];
    a.prefix_group[1] = plan.prefix_group[1];
  }
  a.flat_slots = 0;
  a.flat_defer = 1;
  for (int p = 0; p < 8; ++p) a.group_size[p] = p < g->n_groups ? (uint32_t)g->sizes[p] : 0;
  a.n_groups = g->n_groups;
  a.max_allele = m->max_allele;
  if (mode & kModeWc) {
    // without missing data every site has n_i = group size: the allele-independent W&C terms are per launch
    uint32_t n8[8];
    bool use8[8];
    for (int i = 0; i < 8; ++i) { n8[i] = i < P ? a.group_size[i] : 0; use8[i] = n8[i] != 0; }
    a.wc_shape[0] = wc_shape<8>(n8, use8);
    int k = 1;
    for (int i = 0; i < P; ++i)
      for (int j = i + 1; j < P; ++j, ++k) {
        const uint32_t pn[2] = {n8[i], n8[j]};
        const bool pu[2] = {true, true};
        a.wc_shape[k] = wc_shape<2>(pn, pu);
      }
    a.wc_live_mask = a.wc_s2ok_mask = 0;
    for (int q = 0; q < k; ++q) {
      if (a.wc_shape[q].live) a.wc_live_mask |= 1u << q;
      if (a.wc_shape[q].s2_ok) a.wc_s2ok_mask |= 1u << q;
    }
  }
  a.part_f64 = b.part_f64;
  a.part_u64 = b.part_u64;
  if (mode & kModeDiversity) {
    if (!harmonic) return fail(FMH_ERR_INVALID, "diversity sweep without a harmonic table");
    a.harmonic = harmonic;
  }
  if (plan.empty) return FMH_OK;
  if (plan.status != FMH_OK) return fail(plan.status, "%s", plan.message);
  a.unroll = plan.unroll;
  a.nvec_pad = plan.nvec_pad;
  if (plan.packed) a.single_trip = plan.single_trip;
  if (plan.defer) {
    a.defer_tiles = plan.defer_tiles;
    a.defer_cap = plan.defer_cap;
    a.defer_offset = plan.defer_offset;
  }
  const bool missing = plan.missing, general = plan.general;
  const size_t smem = plan.smem;
  int grid = 0;
  int rc = FMH_OK;
  switch (plan.route) {  // the route's own launcher (sweep_*.hip)
    case SweepRoute::tiled: rc = launch_sweep_tiled(P, mode, a, st, ctx, &grid); break;
    case SweepRoute::flat: rc = launch_sweep_flat(P, mode, a, st, ctx, &grid); break;
    case SweepRoute::mfma: rc = launch_sweep_mfma(P, mode, a, smem, st, ctx, &grid); break;
    case SweepRoute::packed4_3p: rc = launch_sweep_packed4_3p(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::packed16_3p: rc = launch_sweep_packed16_3p(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::packed4: rc = launch_sweep_packed4(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::packed16: rc = launch_sweep_packed16(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::global: rc = launch_sweep_global(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::bits: rc = launch_sweep_bits(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::bytes: rc = launch_sweep_bytes(P, mode, missing, general, a, smem, st, ctx, &grid); break;
    case SweepRoute::none: return fail(FMH_ERR_INVALID, "sweep plan without a route");
  }
  FMH_TRY(rc);
  hipStream_t fin = st;
  if (b.finalize_stream && b.swept) {
    HIP_TRY(hipEventRecord(b.swept, st));
    HIP_TRY(hipStreamWaitEvent(b.finalize_stream, b.swept, 0));
    fin = b.finalize_stream;
  }
  FMH_TRY(launch_finalize(b.part_f64, b.part_u64, grid, b.out_f64, b.out_u64, fin));
  *launched = true;
  return FMH_OK;
}

int fmhi::run_sweep(const fmh_matrix* m, const fmh_groups* g, int mode, SweepArgs& a, void* stream, SweepResult* res) {
  if (!m || !g) return fail(FMH_ERR_INVALID, "matrix or groups is NULL");
  FMH_TRY(use_device(m->device));
  Workspace* w = nullptr;
  FMH_TRY(workspace(m->device, &w));
  LeaseHolder hold;
  hold.w = w;
  FMH_TRY(lease_acquire(w, &hold.l));
  SweepLease* l = hold.l;
  // The caller's stream, or - for the NULL stream - the lease's own (blocking: ordered against the legacy default stream like the NULL
  // stream itself, but not against the other leases), so that sweeps of different host threads (run_vcf's region workers) overlap on the device.
  hipStream_t st = stream ? (hipStream_t)stream : l->stream;
  const bool timing = timing_enabled();  // one snapshot per sweep: another thread may flip the switch while this one runs
  const double* harmonic = nullptr;
  if (mode & kModeDiversity) {
    std::lock_guard<std::mutex> grow(w->in_use);
    FMH_TRY(ensure_harmonic(w, m->columns + 1, st));
    harmonic = w->harmonic;
  }
  memset(res, 0, sizeof *res);
  const LaunchCtx ctx{w->cus, w->max_grid, l->ev0, l->ev1, timing};
  // finalize_kernel writes the 64 + 64 totals straight into the lease's PINNED host vectors (device-visible): a blocking sweep is then two
  // launches and one stream synchronisation.  (Two hipMemcpyAsync of 512 B behind the kernels cost more than the kernels on a small cohort:
  // a lone 512-byte copy_to_host is 22 us on the GPU box, tools/measure_call_overheads.py.)
  const SweepBuffers bufs{l->part_f64, l->part_u64, l->h_f64, l->h_u64};
  bool launched = false;
  FMH_TRY(enqueue_sweep(m, g, mode, a, st, ctx, bufs, harmonic, &launched));
  if (!launched) return FMH_OK;
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(res->f64, l->h_f64, sizeof res->f64);
  memcpy(res->u64, l->h_u64, sizeof res->u64);
  if (timing) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, l->ev0, l->ev1) == hipSuccess) timing_add(ms);  // a timing failure never fails a sweep that has its results
    else (void)hipGetLastError();
  }
  return FMH_OK;
}
