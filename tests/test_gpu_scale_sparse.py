"""Full-scale oracle gates for what run_vcf computes per region: the sparse Hudson formula set (hudson_site_from_variant), the per-site
diversity of both groups (calculate_per_site_diversity) and the fused region sweep (fmh_pair_region_sweep) with run_vcf's pair of formula
sets (DENSE population summaries, SPARSE Hudson) and with SPARSE for both, also sharded over three host-transport ranks.

Every cohort is built on the host by helpers.build_cohort, the builder of tests/test_gpu_scale_general.py (biallelic counter-based rows,
seeded multi-allelic rows, gap rows with the special cases of a population with one call and one with none), or generated on the device and
regenerated on the host, and compared with oracle/dense.py's region_sweep on the same bytes: per-site f64 tracks bit for bit, counts exactly, regional sums to
1e-9.  Every per-site array read from the GPU is compared with an oracle array.  Before any comparison the oracle's own output must show at
least 50 sites of each edge the gap rows are there for: a group with fewer than two calls, a group with no call (D_xy undefined), theta 0
with two or more calls, and FST undefined with num = den = 0."""

import ctypes as C
import functools
import threading
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import dense as D
from tests import helpers as H
from tests.helpers import build_cohort, thresholds

pytestmark = pytest.mark.gpu

TRACKS = ("fst", "dxy", "pi1", "pi2", "num", "den")
HUD_SUMS = ("site_num_sum", "site_den_sum", "site_dxy_sum")
HUD_COUNTS = ("sites_with_components", "site_dxy_skipped")
SUMMARY_SUMS = ("numerator_sum", "denominator_sum", "pi1_sum", "pi2_sum", "dxy_sum_all")  # aggregate_hudson_components_from_summaries: biallelic
EDGE_MIN = 50


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


COHORTS = {
    # rows, samples, multi-allelic fraction, max_allele, gap-row fraction, rows monomorphic in both groups, uploads again with
    "S": (1_000_000, 500, 0.0, 1, 0.002, 0, ()),                                # sparse row_gap, MISSING kernels, four-lane rows
    "M": (1_000_000, 500, 0.02, 7, 0.002, 0, ("FMH_ROW_HI=0", "FMH_LAYOUT=bytes")),  # three planes, GENERAL + MISSING, u8 per-allele fallback
    "W": (250_000, 2500, 0.02, 3, 0.005, 60, ()),                               # sixteen-lane rows
    "X1": (16_000, 90_000, 0.0, 1, 0.02, 60, ()),                               # 180 000 columns: bit masks in LDS
    "X2": (12_000, 100_000, 0.0, 1, 0.02, 60, ()),                              # 200 000 columns: masks past the LDS budget, global-mask route
}


def seed_of(name):
    return 7919 * (ord(name[0]) - 64) + (int(name[1:]) if len(name) > 1 else 0)


def groups_of(N):
    """Population 1 = samples [0, cut), population 2 = [cut, N - 1) (build_cohort's layout)."""
    cut = 2 * N // 5
    Hc = 2 * N
    return cut, np.arange(0, 2 * cut), np.arange(2 * cut, Hc - 2)


def slice_words(words, Hc, b, e):
    """The missing words of rows [b, e) as a matrix of their own."""
    if words is None:
        return None
    lo, hi = b * Hc, e * Hc
    w0, w1 = lo // 64, (hi + 63) // 64
    bits = np.unpackbits(np.ascontiguousarray(words[w0:w1]).view(np.uint8), bitorder="little")[lo - 64 * w0:hi - 64 * w0]
    out = np.packbits(bits, bitorder="little")
    return np.frombuffer(np.pad(out, (0, (-out.size) % 8)).tobytes(), dtype="<u8").copy()


def add_monomorphic(data, words, Hc, cols, count, max_allele, seed, keep):
    """`count` seeded rows without an uncalled column set to one allele (0, 1 or max_allele in turn) in every column of both groups:
    D_xy 0 and pi 0 in both, so FST is undefined with num = den = 0.  With a thousand haplotypes per group two groups are almost never
    monomorphic for the same allele on their own."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in rng.permutation(data.shape[0]):
        if r in keep or (words is not None and slice_words(words, Hc, r, r + 1).any()):
            continue
        rows.append(r)
        if len(rows) == count:
            break
    for i, r in enumerate(rows):
        data[r, cols] = (0, 1, max_allele)[i % 3]
    return np.array(rows)


@functools.lru_cache(maxsize=1)
def cohort(name):
    S, N, frac_multi, max_allele, frac_gap, n_mono, _ = COHORTS[name]
    cut, c1, c2 = groups_of(N)
    data, words, multi = build_cohort(S, N, seed_of(name), frac_multi, max_allele, frac_gap, cut)
    if n_mono:
        add_monomorphic(data, words, 2 * N, np.concatenate([c1, c2]), n_mono, max_allele, seed_of(name) + 1, set(multi[:1].tolist()))
    return data, words


@dataclass
class Expected:
    sites: D.RegionOut   # summary SPARSE, Hudson SPARSE: every per-site array
    pop: dict            # summary formula -> the two groups' totals
    all_pop: dict        # one group of every column (the cohort-wide segregating sites), SPARSE
    hud: dict            # the Hudson fields of fmh_hudson_totals


def oracle(flat, words, S, Hc, declared, off1, off2):
    sp = D.region_sweep(flat, words, S, Hc, declared, off1, off2, D.FORMULA_SPARSE, D.FORMULA_SPARSE, 16)
    de = D.region_sweep(flat, words, S, Hc, declared, off1, off2, D.FORMULA_DENSE, -1, 16)
    every = np.arange(Hc)
    al = D.region_sweep(flat, words, S, Hc, declared, every, every, D.FORMULA_SPARSE, -1, 16)
    return Expected(sp, {D.FORMULA_SPARSE: sp.pop, D.FORMULA_DENSE: de.pop}, al.pop[0], sp.totals)


def add_totals(acc, e):
    """acc += the totals of the next slab (in slab order)."""
    if acc is None:
        return Expected(None, {f: [dict(p) for p in v] for f, v in e.pop.items()}, dict(e.all_pop), dict(e.hud))
    for f in acc.pop:
        for p in range(2):
            for k in ("segregating_sites", "uncallable_sites", "pi_sum"):
                acc.pop[f][p][k] += e.pop[f][p][k]
    for k in ("segregating_sites", "uncallable_sites", "pi_sum"):
        acc.all_pop[k] += e.all_pop[k]
    for k in acc.hud:
        acc.hud[k] += e.hud[k]
    return acc


def edge_counts(e):
    """The edges the gap rows (and the monomorphic rows) are there for, counted in the oracle's own output."""
    return {"n < 2": int(((e.called[0] < 2) | (e.called[1] < 2)).sum()),
            "no call": int(np.isnan(e.dxy).sum()),
            "theta 0, n >= 2": int(((e.called >= 2) & (e.site_theta == 0.0)).any(axis=0).sum()),
            "num = den = 0": int(((e.num == 0.0) & (e.den == 0.0)).sum())}


def check_edges(e, what):
    counts = edge_counts(e)
    print(what, counts)
    for k, v in counts.items():
        assert v >= EDGE_MIN, (what, k, v)


def fused(dev, dm, g2, r0, rows, summary_formula):
    """fmh_pair_region_sweep through ctypes with the sparse Hudson formula set: every track and the totals."""
    from ferromic_amd import _abi

    bufs = {k: dev.DeviceBuffer(dm.device, 16 * rows) for k in ("pi", "theta")}
    bufs.update({k: dev.DeviceBuffer(dm.device, 8 * rows) for k in TRACKS + ("alt", "called")})
    div = _abi.PairDiversitySites(bufs["pi"].ptr, bufs["theta"].ptr)
    sites = _abi.HudsonSites(*(bufs[k].ptr for k in TRACKS + ("alt", "called")))
    tot = _abi.HudsonTotals()
    _abi.check(_abi.load().fmh_pair_region_sweep(dm._h, g2._h, r0, rows, summary_formula, dev.FORMULA_SPARSE, C.byref(div), C.byref(sites),
                                                 C.byref(tot), None))
    return unpack_fused(dev, bufs, tot, rows)


def unpack_fused(dev, bufs, tot, rows):
    out = {"sites": {k: bufs[k].to_numpy(np.float64, rows) for k in TRACKS}}
    for k in ("alt", "called"):
        out["sites"][k] = bufs[k].to_numpy(np.uint32, 2 * rows).reshape(2, rows)
    for k in ("pi", "theta"):
        out[k] = bufs[k].to_numpy(np.float64, 2 * rows).reshape(2, rows)
    out["totals"] = dev.hudson_totals_dict(tot)
    out["pop"] = [{k: getattr(tot.pop[p], k) for k in ("haplotype_capacity", "segregating_sites", "uncallable_sites", "pi_sum")}
                  for p in range(2)]
    for b in bufs.values():
        b.free()
    return out


def gpu_routes(dev, dm, masks, r0, rows):
    """(a) the sparse Hudson sweep, (b) both groups' diversity, (c) the sparse summaries and the one-group summary of every column,
    (d) the fused sweep with run_vcf's pair (DENSE summaries, SPARSE Hudson) and with SPARSE for both."""
    g2 = dev.Groups(dm, masks)
    g1 = [dev.Groups(dm, masks[p:p + 1]) for p in range(2)]
    gall = dev.Groups(dm, np.ones((1, dm.columns), dtype=np.uint8))
    return {"hud": dev.hudson_sweep(dm, g2, dev.FORMULA_SPARSE, r0, rows),
            "div": [dev.diversity_sites(dm, g, r0, rows) for g in g1],
            "ps": dev.population_summaries(dm, g2, dev.FORMULA_SPARSE, r0, rows),
            "all": dev.population_summaries(dm, gall, dev.FORMULA_SPARSE, r0, rows, want_sites=False),
            "fused": {f: fused(dev, dm, g2, r0, rows, f) for f in (dev.FORMULA_DENSE, dev.FORMULA_SPARSE)}}


def check_hudson_sites(sites, e, sl, bi, what):
    for k in TRACKS:
        H.assert_bits_equal(sites[k][sl], getattr(e, k), f"{k} {what}")
    assert np.array_equal(sites["called"][:, sl], e.called), what
    if bi:  # (on a multi-allelic matrix the sweeps' alt counts allele 1, the oracle's gather sums the allele values)
        assert np.array_equal(sites["alt"][:, sl], e.alt), what


def check_fused_sites(fu, e, sl, bi, what):
    check_hudson_sites(fu["sites"], e, sl, bi, what)
    for p in range(2):
        H.assert_bits_equal(fu["pi"][p, sl], e.site_pi[p], f"site pi group {p} {what}")
        H.assert_bits_equal(fu["theta"][p, sl], e.site_theta[p], f"site theta group {p} {what}")


def check_sites(got, e, sl, bi, what):
    """Every per-site array of every route, at rows `sl` of the GPU's arrays, against the oracle's arrays `e`."""
    check_hudson_sites(got["hud"].sites, e, sl, bi, f"hudson_sweep {what}")
    for f, fu in got["fused"].items():
        check_fused_sites(fu, e, sl, bi, f"fused, summary formula {f}, {what}")
    for p in range(2):
        dv = got["div"][p]
        H.assert_bits_equal(dv.pi[sl], e.site_pi[p], f"diversity_sites pi group {p} {what}")
        H.assert_bits_equal(dv.theta[sl], e.site_theta[p], f"diversity_sites theta group {p} {what}")
        assert np.array_equal(dv.called[sl], e.called[p]) and np.array_equal(dv.distinct[sl], e.distinct[p]), (p, what)
    assert np.array_equal(got["ps"].called[:, sl], e.called), what
    if bi:
        assert np.array_equal(got["ps"].alt[:, sl], e.alt), what


def check_pop(got, exp, what):
    for k in ("haplotype_capacity", "segregating_sites", "uncallable_sites"):
        assert got[k] == exp[k], (k, got[k], exp[k], what)
    assert H.rel_close(got["pi_sum"], exp["pi_sum"]), (got["pi_sum"], exp["pi_sum"], what)


def check_hud_totals(got, exp, bi, what):
    for k in HUD_SUMS + (SUMMARY_SUMS if bi else ()):
        assert H.rel_close(got[k], exp[k]), (k, got[k], exp[k], what)
    for k in HUD_COUNTS + (("dxy_uncallable_sites",) if bi else ()):
        assert got[k] == exp[k], (k, got[k], exp[k], what)


def check_fused_totals(fu, exp, f, bi, what):
    for p in range(2):
        check_pop(fu["pop"][p], exp.pop[f][p], f"pop {p} {what}")
    check_hud_totals(fu["totals"], exp.hud, bi, what)


def check_totals(got, exp, bi, what):
    for p in range(2):
        check_pop(got["hud"].pop[p], exp.pop[D.FORMULA_SPARSE][p], f"hudson_sweep pop {p} {what}")
        check_pop(got["div"][p].totals, exp.pop[D.FORMULA_SPARSE][p], f"diversity_sites group {p} {what}")
        check_pop(got["ps"].totals[p], exp.pop[D.FORMULA_SPARSE][p], f"population_summaries group {p} {what}")
    check_pop(got["all"].totals[0], exp.all_pop, f"every column {what}")
    check_hud_totals(got["hud"].totals, exp.hud, bi, f"hudson_sweep {what}")
    for f, fu in got["fused"].items():
        check_fused_totals(fu, exp, f, bi, f"fused, summary formula {f}, {what}")


def sub_range(S):
    """(e): a row range from an unaligned row_begin that ends inside a 64-row tile."""
    r0, rows = 64 * (S // 8 // 64) + 37, S // 4 + 13
    assert r0 % 64 and (r0 + rows) % 64 and r0 + rows <= S
    return r0, rows


@pytest.mark.parametrize("name", list(COHORTS))
def test_cohort_against_c_oracle(dev, fmh_opts, name):
    S, N, _, max_allele, _, _, again = COHORTS[name]
    Hc = 2 * N
    _, off1, off2 = groups_of(N)
    data, words = cohort(name)
    flat = data.reshape(-1)
    bi = max_allele <= 1
    exp = oracle(flat, words, S, Hc, max_allele, off1, off2)
    check_edges(exp.sites, f"cohort {name}")
    r0, rows = sub_range(S)
    exp_sub = oracle(data[r0:r0 + rows].reshape(-1), slice_words(words, Hc, r0, r0 + rows), rows, Hc, max_allele, off1, off2)
    masks = np.zeros((2, Hc), dtype=np.uint8)
    masks[0, off1], masks[1, off2] = 1, 1
    for opt in (None,) + again:
        if opt is not None:
            fmh_opts.setenv(*opt.split("="))
        what = f"cohort {name}" + (f" {opt}" if opt else "")
        dm = dev.DeviceMatrix.from_host(flat, words, S, N, 2, max_allele)
        assert dm.max_allele == max_allele
        got = gpu_routes(dev, dm, masks, 0, S)
        check_sites(got, exp.sites, slice(0, S), bi, what)
        check_totals(got, exp, bi, what)
        del got
        g2 = dev.Groups(dm, masks)
        sub = fused(dev, dm, g2, r0, rows, dev.FORMULA_DENSE)
        check_fused_sites(sub, exp_sub.sites, slice(0, rows), bi, f"fused rows [{r0}, {r0 + rows}) {what}")
        check_fused_totals(sub, exp_sub, D.FORMULA_DENSE, bi, f"fused rows [{r0}, {r0 + rows}) {what}")
        dm.close()
        if opt is not None:
            fmh_opts.delenv(opt.split("=")[0])


def test_cohort_B_device_generated(dev):
    """2 M sites x 5 000 haplotypes, biallelic, nothing missing, generated and packed on the device: the no-missing arm of the DENSE
    summary next to the sparse Hudson pi in the fused sweep.  The oracle regenerates the cohort on the host slab by slab."""
    S, N = 2_000_000, 2500
    seed = seed_of("B")
    Hc = 2 * N
    _, off1, off2 = groups_of(N)
    thr = thresholds(S, seed)
    poc = np.repeat((np.arange(N) >= N // 2).astype(np.uint8), 2)
    dm = dev.DeviceMatrix.alloc(S, N, 2, with_missing=False)
    dm.generate(seed, 0, thr, poc, 0)
    dm.pack(release_bytes=True)
    masks = np.zeros((2, Hc), dtype=np.uint8)
    masks[0, off1], masks[1, off2] = 1, 1
    got = gpu_routes(dev, dm, masks, 0, S)
    r0, rows = sub_range(S)
    sub = fused(dev, dm, dev.Groups(dm, masks), r0, rows, dev.FORMULA_DENSE)

    def host(b, e):
        data, _ = D.generate(e - b, Hc, seed, b, np.ascontiguousarray(thr[:, b:e]), poc, 0, 16)
        return oracle(data, None, e - b, Hc, 1, off1, off2)

    acc = None
    slab = 500_000
    for b in range(0, S, slab):
        e = min(S, b + slab)
        ex = host(b, e)
        check_sites(got, ex.sites, slice(b, e), True, f"cohort B slab {b}")
        acc = add_totals(acc, ex)
    check_totals(got, acc, True, "cohort B")
    ex = host(r0, r0 + rows)
    check_fused_sites(sub, ex.sites, slice(0, rows), True, f"cohort B fused rows [{r0}, {r0 + rows})")
    check_fused_totals(sub, ex, D.FORMULA_DENSE, True, f"cohort B fused rows [{r0}, {r0 + rows})")
    dm.close()


def test_sharded_fused_sweep_cohort_S(dev):
    """fmh_pair_region_sweep_sharded (run_vcf's pair) on cohort S over three host-transport ranks, each with its own slab of a row count
    that three does not divide: every rank's tracks are the oracle's slice bit for bit, the all-rank totals the oracle's whole-cohort
    totals to 1e-9."""
    from ferromic_amd import _abi, sharding

    lib = _abi.load()
    S, N, _, max_allele, _, _, _ = COHORTS["S"]
    assert S % 3 != 0
    Hc = 2 * N
    _, off1, off2 = groups_of(N)
    data, words = cohort("S")
    exp = oracle(data.reshape(-1), words, S, Hc, max_allele, off1, off2)
    masks = np.zeros((2, Hc), dtype=np.uint8)
    masks[0, off1], masks[1, off2] = 1, 1
    ranks = 3
    comms = sharding.Comm.init_all([0] * ranks)
    assert all(c.transport == "host" and c.world == ranks for c in comms)
    out, errors = [None] * ranks, []

    def work(r):
        try:
            b, e = sharding.slab_for_rank(S, r, ranks)
            dm = dev.DeviceMatrix.from_host(data[b:e], slice_words(words, Hc, b, e), e - b, N, 2, max_allele)
            g2 = dev.Groups(dm, masks)
            rows = e - b
            bufs = {k: dev.DeviceBuffer(dm.device, 16 * rows) for k in ("pi", "theta")}
            bufs.update({k: dev.DeviceBuffer(dm.device, 8 * rows) for k in TRACKS + ("alt", "called")})
            div = _abi.PairDiversitySites(bufs["pi"].ptr, bufs["theta"].ptr)
            sites = _abi.HudsonSites(*(bufs[k].ptr for k in TRACKS + ("alt", "called")))
            tot = _abi.HudsonTotals()
            _abi.check(lib.fmh_pair_region_sweep_sharded(comms[r]._h, dm._h, g2._h, 0, rows, dev.FORMULA_DENSE, dev.FORMULA_SPARSE,
                                                         C.byref(div), C.byref(sites), C.byref(tot), None))
            out[r] = (b, e, unpack_fused(dev, bufs, tot, rows))
            dm.close()
        except Exception as exc:  # noqa: BLE001 - reported by the main thread
            errors.append((r, exc))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for c in comms:
        c.close()
    for r in range(ranks):
        b, e, fu = out[r]
        part = D.RegionOut(*(getattr(exp.sites, k)[..., b:e] for k in ("alt", "called", "distinct", "site_pi", "site_theta") + TRACKS),
                           pop=None, totals=None)
        check_fused_sites(fu, part, slice(0, e - b), True, f"rank {r} rows [{b}, {e})")
        check_fused_totals(fu, exp, D.FORMULA_DENSE, True, f"rank {r}, all ranks' totals")
