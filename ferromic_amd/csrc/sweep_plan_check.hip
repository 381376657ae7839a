// sweep_plan_check.hip — prints the plan (sweep_plan.hpp) of a fixed list of sweeps, one tab-separated line per case with every field of
// the plan; tests/test_sweep_plan_cpu.py compares the output with tests/sweep_plans.tsv line by line.  `sweep_plan_check prefix` prints the
// table form's cases instead (plan_prefix: groups given as column ranges on matrices that hold the prefix counts), which
// tests/test_prefix_plan_cpu.py checks against the definition.  The handles are built on the host
// with dummy device pointers that are never dereferenced, and no HIP runtime call is made: the program runs on a machine without a GPU.
// `make plan_check` builds it; the expected table was produced by the decision code as it stood before the plan existed.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "sweep_plan.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

uint8_t* const kPtr = (uint8_t*)(uintptr_t)0x1000;  // "present": never dereferenced

enum Layout { kPackedOnly, kBytesOnly, kBoth };
struct MatrixSpec {
  Layout layout;
  int max_allele;
  bool called;
  uint32_t pvec;  // row width in 128-column vectors; the row ends 5 columns short of the last vector's end
  bool p0t = true, row_alt = true;
};
fmh_matrix make_matrix(const MatrixSpec& s) {
  fmh_matrix m;
  m.columns = s.pvec * 128 - 5;
  m.samples = m.columns;
  m.ploidy = 1;
  m.variants = 100000;
  m.nvec = (m.columns + 15) / 16;
  m.pitch = (size_t)m.nvec * 16;
  m.max_allele = (uint8_t)s.max_allele;
  m.has_missing = s.called;
  if (s.layout != kPackedOnly) {
    m.data = kPtr;
    m.bits = s.called ? kPtr : nullptr;
    m.bits_pitch = s.called ? (size_t)m.nvec * 2 : 0;
  }
  if (s.layout != kBytesOnly) {
    m.pvec = s.pvec;
    m.plane_pitch = (size_t)s.pvec * 16;
    m.p0 = kPtr;
    m.p1 = s.max_allele >= 2 ? kPtr : nullptr;
    m.p2 = s.max_allele >= 4 ? kPtr : nullptr;
    m.pc = s.called ? kPtr : nullptr;
    m.row_gap = s.called ? kPtr : nullptr;
    m.row_hi = s.max_allele >= 2 ? kPtr : nullptr;
    const bool plain = s.max_allele <= 1 && !s.called;  // what the library keeps row totals and the tiled image for
    m.row_alt = plain && s.row_alt ? (uint32_t*)kPtr : nullptr;
    m.p0t = plain && s.p0t ? kPtr : nullptr;
    m.p0t_bytes = m.p0t ? (size_t)1 << 20 : 0;
  }
  return m;
}

// where the groups' members lie, in vectors of a W-vector row
enum Geometry { kPartition, kDisjointGaps, kOverlapping, kInterleaved, kEmptyGroup, kAtStart, kInMiddle, kAtEnd, kSevenEighths, kSevenEighthsPlusOne, kGeometries };
const char* const kGeometryName[kGeometries] = {"partition", "gaps", "overlap", "interleaved", "emptygroup", "start", "middle", "end", "7of8", "7of8+1"};

fmh_groups make_groups(const fmh_matrix& m, uint32_t W, int n, Geometry geo, bool mask_flat) {
  fmh_groups g;
  g.n_groups = n;
  g.padded = n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : 8;
  g.masks = kPtr;
  g.mask_bits = (uint16_t*)kPtr;
  g.mask_flat = mask_flat && W <= 32 ? (uint32_t*)kPtr : nullptr;
  g.pitch = m.pitch;
  g.mask_pitch = (m.pitch + 2047) / 2048 * 2048;
  g.columns = m.columns;
  auto span = [&](uint32_t lo, uint32_t hi) {  // every group inside [lo, hi], side by side where the range has room
    const uint32_t len = hi - lo + 1;
    for (int i = 0; i < n; ++i) {
      g.vec_first[i] = lo + (uint32_t)((uint64_t)len * i / n);
      const uint32_t next = lo + (uint32_t)((uint64_t)len * (i + 1) / n);
      g.vec_last[i] = next > g.vec_first[i] ? next - 1 : g.vec_first[i];
    }
  };
  for (int i = 0; i < n; ++i) g.sizes[i] = 10 + 3 * i;
  g.disjoint = true;
  g.covers = false;
  switch (geo) {
    case kPartition:
      span(0, W - 1);
      g.covers = true;
      break;
    case kDisjointGaps:
      span(0, W - 1);
      if (W >= 3) { g.vec_first[0] += 1; g.vec_last[n - 1] -= g.vec_last[n - 1] > g.vec_first[n - 1] ? 1 : 0; }
      break;
    case kOverlapping:
      for (int i = 0; i < n; ++i) { g.vec_first[i] = 0; g.vec_last[i] = W - 1; }
      g.disjoint = false;
      g.covers = true;
      break;
    case kInterleaved:
      for (int i = 0; i < n; ++i) { g.vec_first[i] = 0; g.vec_last[i] = W - 1; }
      g.covers = true;
      break;
    case kEmptyGroup:
      span(0, W - 1);
      g.vec_first[n - 1] = 1;
      g.vec_last[n - 1] = 0;
      g.sizes[n - 1] = 0;
      break;
    case kAtStart: span(0, W / 4); break;
    case kInMiddle: span(W / 3, 2 * W / 3); break;
    case kAtEnd: span(W - 1 - W / 4, W - 1); break;
    case kSevenEighths: span(0, W * 7 / 8 - 1); break;
    case kSevenEighthsPlusOne: span(0, W * 7 / 8); break;
    default: break;
  }
  return g;
}

const char* route_name(SweepRoute r) {
  static const char* const names[] = {"none", "tiled", "flat", "mfma", "packed4", "packed16", "packed4_3p", "packed16_3p", "global", "bits", "bytes"};
  return names[(int)r];
}

const LdsFigures kLds160{150 * 1024, 160 * 1024};  // gfx950: 160 KiB per CU, 150 of them for masks
const LdsFigures kLds64{150 * 1024, 64 * 1024};    // a runtime that reports 64 KiB: the mask limit falls back to 150 KiB, a CU's LDS is what was reported

size_t g_cases = 0;
void print_case(const std::string& name, const fmh_matrix& m, const fmh_groups& g, int mode, size_t row_count, const PlanOptions& o, const LdsFigures& lds) {
  const SweepPlan p = plan_sweep(m, g, mode, row_count, o, lds);
  // the probes' fields and the helpers' answers hold for every case; the launch fields only for a plan that launches
  printf("%s\t%d\t%s\t%d\t%u\t%u\t%d\t%d\t%d\t%d\t%d", name.c_str(), p.status, p.message[0] ? p.message : "-", (int)p.empty, p.win.first, p.win.count, p.win.derived, (int)p.tiled,
         plan_wc_groups(m, g, o), (int)plan_wc_fused(m, g, lds.limit), (int)plan_summaries_single(m, g, lds.limit));
  if (p.status == FMH_OK && !p.empty)
    printf("\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%u\t%d\t%zu\t%d\t%d\t%d\t%u\n", (int)p.packed, p.P, (int)p.missing, (int)p.general, (int)p.windowed, route_name(p.route), p.lpr, p.unroll, p.nvec_pad,
           (int)p.single_trip, p.smem, (int)p.defer, p.defer_tiles, p.defer_cap, p.defer_offset);
  else printf("\t-\n");
  ++g_cases;
}

std::string matrix_name(const MatrixSpec& s, long long layout_bytes) {
  char buf[96];
  snprintf(buf, sizeof buf, "%s%s/a%d/c%d/w%u/t%d%d", s.layout == kPackedOnly ? "packed" : s.layout == kBytesOnly ? "u8" : "both", layout_bytes ? "+bytes" : "", s.max_allele,
           (int)s.called, s.pvec, (int)s.p0t, (int)s.row_alt);
  return buf;
}

struct Sweep {
  int groups, mode;
};
const int S = kModeSummary, SH = kModeSummary | kModeHudson, SD = kModeSummary | kModeDiversity, SHD = kModeSummary | kModeHudson | kModeDiversity, WC = kModeWc;
// every group count with every mode it is valid in, the group counts each mode refuses, and two modes that do not exist
const Sweep kSweeps[] = {{1, S}, {2, S}, {3, S}, {4, S}, {5, S}, {6, S}, {7, S}, {8, S}, {2, SH}, {1, SD}, {2, SD}, {2, SHD}, {2, WC}, {3, WC},
                         {4, WC}, {5, WC}, {6, WC}, {7, WC}, {8, WC}, {1, SH}, {3, SH}, {4, SD}, {1, SHD}, {1, WC}, {2, 16}, {2, S | WC}, {4, 0}};
const int kNSweeps = (int)(sizeof kSweeps / sizeof kSweeps[0]);
const uint32_t kWidths[] = {1, 4, 8, 9, 20, 21, 32, 33, 40, 64, 1563};

void run(const char* set, const MatrixSpec& ms, const Sweep& sw, Geometry geo, bool mask_flat, size_t row_count, const PlanOptions& o, const char* opt_name, const LdsFigures& lds) {
  const fmh_matrix m = make_matrix(ms);
  const fmh_groups g = make_groups(m, ms.pvec, sw.groups, geo, mask_flat);
  char tail[128];
  snprintf(tail, sizeof tail, "/g%d/m%d/%s/f%d/r%zu/%s/lds%zu", sw.groups, sw.mode, kGeometryName[geo], (int)mask_flat, row_count, opt_name, lds.per_cu / 1024);
  print_case(std::string(set) + "/" + matrix_name(ms, o.layout_bytes) + tail, m, g, sw.mode, row_count, o, lds);
}

// ---- the table form (plan_prefix): groups as column ranges [c0, c1), several ranges = a group that is not contiguous -----------------------
struct Range {
  uint32_t c0, c1;
};
struct RangeGroup {
  std::vector<Range> ranges;
};
fmh_groups make_range_groups(const fmh_matrix& m, const std::vector<RangeGroup>& gs) {
  fmh_groups g;
  const int n = (int)gs.size();
  g.n_groups = n;
  g.padded = n <= 1 ? 1 : 2;
  g.masks = kPtr;
  g.mask_bits = (uint16_t*)kPtr;
  g.pitch = m.pitch;
  g.mask_pitch = (m.pitch + 2047) / 2048 * 2048;
  g.columns = m.columns;
  std::vector<int> seen(m.columns, 0);
  for (int i = 0; i < n; ++i) {
    uint32_t lo = UINT32_MAX, hi = 0, size = 0;
    for (const Range& r : gs[i].ranges) {
      lo = std::min(lo, r.c0);
      hi = std::max(hi, r.c1);
      size += r.c1 - r.c0;
      for (uint32_t c = r.c0; c < r.c1; ++c) ++seen[c];
    }
    g.sizes[i] = size;
    g.vec_first[i] = lo / 128;
    g.vec_last[i] = (hi - 1) / 128;
    g.col_first[i] = lo;
    g.col_end[i] = hi;
    g.contiguous[i] = size == hi - lo;
  }
  g.disjoint = g.covers = true;
  for (int s : seen) {
    if (s > 1) g.disjoint = false;
    if (s == 0) g.covers = false;
  }
  return g;
}
void print_prefix_case(const char* what, uint32_t W, const std::vector<RangeGroup>& gs, int mode, const PlanOptions& o, bool table) {
  fmh_matrix m = make_matrix(MatrixSpec{kPackedOnly, 1, false, W});
  m.p0c = table ? (uint16_t*)kPtr : nullptr;
  m.p0c_bytes = table ? 1 : 0;
  const fmh_groups g = make_range_groups(m, gs);
  const SweepPlan p = plan_sweep(m, g, mode, 5000, o, kLds160);
  std::string name = std::string(what) + "/w" + std::to_string(W) + "/c" + std::to_string(m.columns) + "/m" + std::to_string(mode) + "/";
  for (size_t i = 0; i < gs.size(); ++i) {
    if (i) name += "|";
    for (size_t k = 0; k < gs[i].ranges.size(); ++k) name += (k ? "+" : "") + std::to_string(gs[i].ranges[k].c0) + "-" + std::to_string(gs[i].ranges[k].c1);
  }
  printf("%s\t%d\t%s\t%d\t%d\t%u\t%u\t%u\t%d", name.c_str(), p.status, route_name(p.route), (int)p.tiled, (int)p.prefix, p.prefix_vecs, p.win.first, p.win.count, p.win.derived);
  const int counted = p.prefix ? g.n_groups - (p.win.derived >= 0 ? 1 : 0) : 0;
  for (int q = 0; q < counted; ++q) {
    const PrefixGroup& pg = p.prefix_group[q];
    printf("\t%u,%u,%u", pg.b_lo, pg.b_hi, pg.n_edges);
    for (int k = 0; k < 2; ++k) printf(",%u:%08x.%08x.%08x.%08x", pg.edge_vec[k], pg.edge_mask[k][0], pg.edge_mask[k][1], pg.edge_mask[k][2], pg.edge_mask[k][3]);
  }
  printf("\n");
  ++g_cases;
}
int prefix_cases() {
  PlanOptions on;
  on.tiled = 1;  // the route wherever it is built: the table form is decided on top of it
  const int one = kModeSummary | kModeDiversity, two = kModeSummary | kModeHudson;
  // 1. the edges first: a range of whole vectors only (no vector read), one that ends / starts on a vector boundary, one column inside it, a
  //    range inside one vector, two adjacent partial vectors with nothing whole between them, the whole row
  for (uint32_t W : {1u, 2u, 3u, 40u}) {
    const uint32_t cols = W * 128 - 5;
    std::vector<Range> rs = {{0, cols}, {0, 1}, {cols - 1, cols}, {3, 100u < cols ? 100u : cols - 1}};
    if (W >= 2) for (Range r : {Range{0, 128}, Range{0, 127}, Range{0, 129}, Range{1, 128}, Range{128, cols}, Range{127, cols}, Range{129, cols}, Range{100, 200}, Range{127, 129}}) rs.push_back(r);
    if (W >= 3) for (Range r : {Range{128, 256}, Range{128, 257}, Range{127, 256}, Range{129, 255}, Range{130, 140}, Range{1, cols - 1}}) rs.push_back(r);
    if (W == 40) for (Range r : {Range{0, 2500}, Range{2500, cols}, Range{1280, 3840}, Range{1281, 3839}, Range{4992, cols}, Range{4991, cols}, Range{4993, cols - 1}}) rs.push_back(r);
    for (const Range& r : rs) print_prefix_case("one", W, {RangeGroup{{r}}}, one, on, true);
    // two groups: a partition (one derived, the other from the table), two ranges with a gap (both counted), ranges that share a vector
    std::vector<std::pair<Range, Range>> pairs = {{{0, cols / 2}, {cols / 2, cols}}, {{0, 64u < cols / 2 ? 64u : 1u}, {cols / 2, cols}}, {{cols / 2, cols}, {0, cols / 2}}};
    if (W >= 2) for (auto pr : {std::pair<Range, Range>{{0, 128}, {128, cols}}, {{0, 100}, {110, 200}}, {{10, 128}, {128, 250}}}) pairs.push_back(pr);
    if (W == 40) for (auto pr : {std::pair<Range, Range>{{0, 2500}, {2500, cols}}, {{0, 2560}, {2560, cols}}, {{100, 1000}, {3000, 4000}}, {{0, 4900}, {4900, cols}}}) pairs.push_back(pr);
    for (const auto& pr : pairs) print_prefix_case("two", W, {RangeGroup{{pr.first}}, RangeGroup{{pr.second}}}, two, on, true);
  }
  // 2. a counted group that is not one range keeps the window, whatever the other one is; a derived one does not matter
  print_prefix_case("split", 40, {RangeGroup{{{0, 100}, {200, 300}}}}, one, on, true);
  print_prefix_case("split", 40, {RangeGroup{{{0, 100}, {200, 300}}}, RangeGroup{{{1000, 2000}}}}, two, on, true);
  print_prefix_case("split", 40, {RangeGroup{{{1000, 2000}}}, RangeGroup{{{0, 1000}, {2000, 5115}}}}, two, on, true);   // the split group is derived
  print_prefix_case("split", 40, {RangeGroup{{{0, 1000}, {2000, 5115}}}, RangeGroup{{{1000, 2000}}}}, two, on, true);
  // 3. no table, the table switched off, the route switched off, the default route rule (seven eighths of the row), W&C
  PlanOptions off = on, untiled = on, dflt;
  off.prefix_counts = 0;
  untiled.tiled = 0;
  const std::vector<RangeGroup> half = {RangeGroup{{{0, 2500}}}, RangeGroup{{{2500, 5115}}}};
  print_prefix_case("notable", 40, half, two, on, false);
  print_prefix_case("off", 40, half, two, off, true);
  print_prefix_case("untiled", 40, half, two, untiled, true);
  print_prefix_case("default", 40, half, two, dflt, true);
  print_prefix_case("default", 40, {RangeGroup{{{0, 2500}}}, RangeGroup{{{2500, 5000}}}}, two, dflt, true);  // 40 of 40 vectors: the row-major route
  print_prefix_case("wc", 40, half, kModeWc, on, true);
  fprintf(stderr, "sweep_plan_check: %zu prefix cases\n", g_cases);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "prefix") return prefix_cases();
  const PlanOptions defaults;
  PlanOptions bytes_forced;
  bytes_forced.layout_bytes = 1;
  // 1. shapes: every layout, allele range, called plane and width with one sweep each (the list rotates: every sweep meets every width)
  int turn = 0;
  for (int layout = 0; layout < 4; ++layout)
    for (int allele : {1, 2, 3, 5})
      for (int called = 0; called < 2; ++called)
        for (uint32_t w : kWidths) {
          const MatrixSpec ms{layout == 0 ? kPackedOnly : layout == 1 ? kBytesOnly : kBoth, allele, called != 0, w};
          run("shape", ms, kSweeps[(turn++ * 7) % kNSweeps], kPartition, true, 5000, layout == 3 ? bytes_forced : defaults, "default", kLds160);
        }
  // 2. every sweep of the list on plain packed and u8 rows of two widths
  for (Layout layout : {kPackedOnly, kBytesOnly})
    for (uint32_t w : {4u, 40u})
      for (const Sweep& sw : kSweeps) run("sweeps", MatrixSpec{layout, 1, false, w}, sw, kPartition, true, 5000, defaults, "default", kLds160);
  // 3. group geometry on plain packed rows (32 and 64 vectors: the seven-eighths rule only); then the tiled image, the row totals and the
  //    flat masks present and absent
  for (uint32_t w : {8u, 32u, 40u, 64u})
    for (int geo = 0; geo < kGeometries; ++geo) {
      if ((w == 32 || w == 64) && geo < kSevenEighths) continue;
      for (const Sweep& sw : {Sweep{1, SD}, Sweep{2, S}, Sweep{2, SH}, Sweep{3, S}}) run("geometry", MatrixSpec{kPackedOnly, 1, false, w}, sw, (Geometry)geo, true, 5000, defaults, "default", kLds160);
    }
  const bool tables[5][3] = {{true, true, true}, {false, true, true}, {true, false, true}, {true, true, false}, {false, false, false}};  // p0t, row_alt, mask_flat
  for (uint32_t w : {8u, 40u})
    for (Geometry geo : {kPartition, kInMiddle})
      for (const Sweep& sw : {Sweep{1, S}, Sweep{2, SHD}})
        for (const auto& t : tables) {
          MatrixSpec ms{kPackedOnly, 1, false, w};
          ms.p0t = t[0];
          ms.row_alt = t[1];
          run("tables", ms, sw, geo, t[2], 5000, defaults, "default", kLds160);
        }
  // 4. every routing option at its default and at each forcing value, one at a time
  struct Setting {
    const char* name;
    long long PlanOptions::*field;
    long long value;
  };
  const Setting settings[] = {
      {"flat=-1", &PlanOptions::flat, -1}, {"flat=0", &PlanOptions::flat, 0}, {"flat=1", &PlanOptions::flat, 1},
      {"tiled=-1", &PlanOptions::tiled, -1}, {"tiled=0", &PlanOptions::tiled, 0}, {"tiled=1", &PlanOptions::tiled, 1},
      {"column_window=0", &PlanOptions::column_window, 0}, {"column_window=1", &PlanOptions::column_window, 1}, {"column_window=2", &PlanOptions::column_window, 2},
      {"counts_mfma=0", &PlanOptions::counts_mfma, 0}, {"counts_mfma=1", &PlanOptions::counts_mfma, 1}, {"counts_mfma=2", &PlanOptions::counts_mfma, 2},
      {"mask_mode=-1", &PlanOptions::mask_mode, -1}, {"mask_mode=0", &PlanOptions::mask_mode, 0}, {"mask_mode=1", &PlanOptions::mask_mode, 1}, {"mask_mode=2", &PlanOptions::mask_mode, 2},
      {"packed_lpr=0", &PlanOptions::packed_lpr, 0}, {"packed_lpr=4", &PlanOptions::packed_lpr, 4}, {"packed_lpr=16", &PlanOptions::packed_lpr, 16},
      {"packed_unroll=0", &PlanOptions::packed_unroll, 0}, {"packed_unroll=1", &PlanOptions::packed_unroll, 1}, {"packed_unroll=2", &PlanOptions::packed_unroll, 2},
      {"packed_unroll=3", &PlanOptions::packed_unroll, 3}, {"packed_unroll=4", &PlanOptions::packed_unroll, 4}, {"packed_unroll=5", &PlanOptions::packed_unroll, 5},
      {"packed_no_prefetch=0", &PlanOptions::packed_no_prefetch, 0}, {"packed_no_prefetch=1", &PlanOptions::packed_no_prefetch, 1},
      {"defer_tiles=0", &PlanOptions::defer_tiles, 0}, {"defer_tiles=1", &PlanOptions::defer_tiles, 1}, {"defer_tiles=7", &PlanOptions::defer_tiles, 7},
      {"defer_tiles=16", &PlanOptions::defer_tiles, 16}, {"defer_tiles=17", &PlanOptions::defer_tiles, 17},
      {"wc_exact=0", &PlanOptions::wc_exact, 0}, {"wc_exact=1", &PlanOptions::wc_exact, 1}, {"unroll=0", &PlanOptions::unroll, 0}, {"unroll=8", &PlanOptions::unroll, 8},
  };
  const struct { MatrixSpec ms; Sweep sw; } opt_cases[] = {
      {{kPackedOnly, 1, false, 8}, {2, SH}}, {{kPackedOnly, 1, false, 20}, {1, S}}, {{kPackedOnly, 1, false, 40}, {2, SHD}}, {{kPackedOnly, 1, false, 40}, {5, WC}},
      {{kPackedOnly, 2, true, 40}, {4, S}}, {{kBytesOnly, 1, false, 8}, {2, SH}}, {{kBytesOnly, 1, false, 8}, {4, S}}, {{kBytesOnly, 1, true, 40}, {8, WC}}};
  for (const Setting& st : settings)
    for (const auto& c : opt_cases) {
      PlanOptions o;
      o.*st.field = st.value;
      run("options", c.ms, c.sw, kAtStart, true, 5000, o, st.name, kLds160);
    }
  // 5. the LDS figures of the 160-KiB device and of the 64-KiB fallback, on widths whose u8 masks fit LDS as bytes, as bits, or not at all
  for (const LdsFigures& lds : {kLds160, kLds64})
    for (uint32_t w : {40u, 1563u, 5469u})
      for (Layout layout : {kBytesOnly, kPackedOnly})
        for (int plain = 0; plain < 2; ++plain)
          for (const Sweep& sw : {Sweep{1, S}, Sweep{2, SH}, Sweep{4, S}, Sweep{8, S}, Sweep{8, WC}})
            run("lds", MatrixSpec{layout, plain ? 1 : 2, plain == 0, w}, sw, kPartition, true, 5000, defaults, "default", lds);
  // 6. an empty row range: nothing is refused, whatever the sweep
  for (Layout layout : {kPackedOnly, kBytesOnly})
    for (const Sweep& sw : {Sweep{2, SH}, Sweep{1, SH}, Sweep{8, S}, Sweep{8, WC}, Sweep{2, 16}}) run("empty", MatrixSpec{layout, 1, false, 5469}, sw, kPartition, true, 0, defaults, "default", kLds160);
  // 7. the opt-in routes forced: where each route is built and where it gives way
  PlanOptions flat_on, tiled_on, both_on, mfma1, mfma2;
  flat_on.flat = both_on.flat = 1;
  tiled_on.tiled = both_on.tiled = 1;
  mfma1.counts_mfma = 1;
  mfma2.counts_mfma = 2;
  const Sweep forced_sweeps[] = {{1, S}, {2, S}, {4, S}, {8, S}, {2, SH}, {1, SD}, {2, SD}, {2, SHD}, {2, WC}, {4, WC}, {5, WC}, {3, SH}};
  const struct { const char* name; const PlanOptions* o; bool packed; } forced[] = {{"flat=1", &flat_on, true}, {"tiled=1", &tiled_on, true}, {"flat=1,tiled=1", &both_on, true},
                                                                                    {"counts_mfma=1", &mfma1, false}, {"counts_mfma=2", &mfma2, false}};
  for (const auto& f : forced)
    for (uint32_t w : {8u, 32u, 33u}) {
      if (!f.packed && w == 32) continue;
      for (const Sweep& sw : forced_sweeps) run("forced", MatrixSpec{f.packed ? kPackedOnly : kBytesOnly, 1, false, w}, sw, kInMiddle, true, 5000, *f.o, f.name, kLds160);
    }
  fprintf(stderr, "sweep_plan_check: %zu cases\n", g_cases);
  return 0;
}
