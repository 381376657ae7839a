"""Pins the C half of the oracle (oracle/dense_oracle.c) to the Python restatement, which is itself
pinned by the reference's own KATs (tests/test_oracle_golden.py)."""

import random

import numpy as np
import pytest

from oracle import dense as D
from oracle import ferromic_ref as R
from tests import helpers as H


@pytest.mark.parametrize("sites,samples,p_missing,threads", [(400, 31, 0.0, 1), (400, 31, 0.0, 3), (333, 26, 0.12, 4)])
def test_c_sweep_matches_python_oracle(sites, samples, p_missing, threads):
    rng = np.random.default_rng(sites + samples)
    m = H.random_dense_matrix(rng, sites, samples, 2, 1, p_missing)
    h1 = H.haps_for_samples(range(0, samples // 2))
    h2 = H.haps_for_samples(range(samples // 2, samples - 1))
    off1 = R.dense_membership_offsets(m, h1)
    off2 = R.dense_membership_offsets(m, h2)
    out = D.hudson_sweep(np.frombuffer(m.data, dtype=np.uint8), H.missing_words_np(m), sites, m.stride, off1, off2, threads)
    s1 = R.build_dense_population_summary(m, h1)
    s2 = R.build_dense_population_summary(m, h2)
    assert np.array_equal(out.alt[0], np.array(s1.alt_counts, dtype=np.uint32))
    assert np.array_equal(out.called[1], np.array(s2.called_counts, dtype=np.uint32))
    assert out.pop[0]["segregating_sites"] == s1.segregating_sites
    assert out.pop[1]["segregating_sites"] == s2.segregating_sites
    assert H.rel_close(out.pop[0]["pi_sum"], s1.pi_sum, 1e-12)
    t = R.aggregate_hudson_components_from_summaries(s1, s2)
    for k in ("numerator_sum", "denominator_sum", "pi1_sum", "pi2_sum", "dxy_sum_all"):
        assert H.rel_close(out.totals[k], getattr(t, k), 1e-12), k
    assert out.totals["dxy_uncallable_sites"] == t.dxy_uncallable_sites
    exp = R.dense_hudson_sites(m, [R.Variant(i, None) for i in range(sites)], off1, off2)
    H.assert_bits_equal(out.fst, [H.opt(x.fst) for x in exp], "fst")
    H.assert_bits_equal(out.dxy, [H.opt(x.d_xy) for x in exp], "dxy")
    H.assert_bits_equal(out.pi1, [H.opt(x.pi_pop1) for x in exp], "pi1")
    H.assert_bits_equal(out.pi2, [H.opt(x.pi_pop2) for x in exp], "pi2")
    H.assert_bits_equal(out.num, [H.opt(x.num_component) for x in exp], "num")
    H.assert_bits_equal(out.den, [H.opt(x.den_component) for x in exp], "den")
    ns, ds = R.hudson_component_sums(exp)
    assert H.rel_close(out.totals["site_num_sum"], ns, 1e-12) and H.rel_close(out.totals["site_den_sum"], ds, 1e-12)


def test_generator_is_deterministic_and_thread_independent():
    S, H_ = 300, 50
    rng = np.random.default_rng(3)
    thr = (rng.random((2, S)) * (1 << 24)).astype(np.uint32)
    poc = (np.arange(H_) >= H_ // 2).astype(np.uint8)
    a, wa = D.generate(S, H_, 99, 1000, thr, poc, int(0.1 * (1 << 24)), 1)
    b, wb = D.generate(S, H_, 99, 1000, thr, poc, int(0.1 * (1 << 24)), 5)
    assert np.array_equal(a, b) and np.array_equal(wa, wb)
    # slab property used for region sharding: rows [100,200) of the cohort == a slab generated alone
    c, wc = D.generate(100, H_, 99, 1100, thr[:, 100:200].copy(), poc, 0, 2)
    c2, _ = D.generate(S, H_, 99, 1000, thr, poc, 0, 2)
    assert np.array_equal(c, c2.reshape(S, H_)[100:200].reshape(-1))
    frac = a.reshape(S, H_)[:, : H_ // 2].mean(axis=1)
    assert abs(np.corrcoef(frac, thr[0] / float(1 << 24))[0, 1]) > 0.8


@pytest.mark.parametrize("sites,samples,G,max_allele,p_missing,ungrouped,threads", [
    (160, 24, 2, 1, 0.0, 0, 1), (140, 31, 4, 1, 0.08, 3, 3), (120, 26, 3, 3, 0.15, 5, 2), (90, 18, 5, 2, 0.5, 2, 4), (40, 9, 2, 1, 0.97, 0, 1),
    # more groups than the fused kernels take, up to a 26-population cohort
    (60, 40, 9, 1, 0.05, 2, 3), (40, 50, 17, 2, 0.0, 0, 2), (30, 60, 26, 1, 0.03, 1, 4)])
def test_c_wc_matches_python_oracle(sites, samples, G, max_allele, p_missing, ungrouped, threads):
    """fo_wc_sites_threaded against calculate_fst_wc_at_site_with_membership / calculate_overall_fst_wc, bit for bit:
    per-site a, b and state of the overall slot and of every pair, and the regional sums (serial, site order)."""
    rng = np.random.default_rng(1000 * sites + samples + G)
    m = H.random_dense_matrix(rng, sites, samples, 2, max_allele, p_missing)
    data = np.frombuffer(m.data, dtype=np.uint8).reshape(sites, 2 * samples)
    words = H.missing_words_np(m)
    miss = np.zeros((sites, 2 * samples), dtype=bool) if words is None else \
        np.unpackbits(words.view(np.uint8), bitorder="little")[: sites * 2 * samples].reshape(sites, 2 * samples).astype(bool)
    # make the dense mask expressible in the sparse model the Python restatement takes: a genotype whose FIRST allele is missing
    # is None as a whole (process.rs:479-496), one whose second allele is missing is a haploid call
    miss[:, 1::2] |= miss[:, 0::2]
    if words is not None:
        bits = np.packbits(miss.reshape(-1), bitorder="little")
        words = np.frombuffer(np.concatenate([bits, np.zeros((-len(bits)) % 8, np.uint8)]).tobytes(), dtype="<u8").copy()
    group_of_sample = rng.integers(0, G, size=samples)
    group_of_sample[:G] = np.arange(G)            # every group has a member
    group_map = {(s, side): str(int(group_of_sample[s])) for s in range(samples - ungrouped) for side in (0, 1)}
    membership = R.SubpopulationMembership.from_map(samples, group_map)
    goc = np.full(2 * samples, 0xFF, dtype=np.uint8)
    for (s, side), label in group_map.items():
        goc[2 * s + side] = membership.labels.index(label)
    n_groups = membership.group_count()
    out = D.wc_sites(data.reshape(-1), words, sites, 2 * samples, goc, n_groups, threads)
    # without per-site arrays: the same informative counts; one thread sums in site order (the same bits), more threads range by range
    for t in (1, threads):
        lean = D.wc_sites(data.reshape(-1), words, sites, 2 * samples, goc, n_groups, t, sites=False)
        assert lean.a is None and np.array_equal(lean.informative, out.informative)
        if t == 1:
            assert np.array_equal(lean.sum_a.view(np.uint64), out.sum_a.view(np.uint64)) and np.array_equal(lean.sum_b.view(np.uint64), out.sum_b.view(np.uint64))
        else:
            assert np.allclose(lean.sum_a, out.sum_a, rtol=1e-12, atol=1e-15) and np.allclose(lean.sum_b, out.sum_b, rtol=1e-12, atol=1e-15)
    pairs = [(i, j) for i in range(n_groups) for j in range(i + 1, n_groups)]
    states = {"calculable": 0, "components_yield_indeterminate_ratio": 1, "no_inter_population_variance": 2, "insufficient_data_for_estimation": 3}
    site_records = []
    for s in range(sites):
        genos = []
        for smp in range(samples):
            g = [int(data[s, 2 * smp + k]) for k in (0, 1)]
            genos.append(None if miss[s, 2 * smp] else (g[:1] if miss[s, 2 * smp + 1] else g))
        overall, pw, comps, sizes, pcomps = R.calculate_fst_wc_at_site_with_membership(R.make_variant(s, genos), membership)
        site_records.append(R.SiteFstWc(s + 1, overall, pw, comps, sizes, pcomps))
        assert (float(out.a[0][s]), float(out.b[0][s])) == comps, s
        assert int(out.state[0][s]) == states[overall.state], s
        for k, (i, j) in enumerate(pairs, start=1):
            key = f"{membership.labels[i]}_vs_{membership.labels[j]}"
            if overall.state == "insufficient_data_for_estimation":
                assert int(out.state[k][s]) == 3
                continue
            assert (float(out.a[k][s]), float(out.b[k][s])) == pcomps[key], (s, key)
            assert int(out.state[k][s]) == states[pw[key].state], (s, key)
    overall, pw, agg = R.calculate_overall_fst_wc(site_records)
    if overall.state != "insufficient_data_for_estimation":
        assert (float(out.sum_a[0]), float(out.sum_b[0])) == (overall.sum_a, overall.sum_b) and int(out.informative[0]) == overall.sites
    for k, (i, j) in enumerate(pairs, start=1):
        key = f"{membership.labels[i]}_vs_{membership.labels[j]}"
        if key in agg and pw[key].state != "insufficient_data_for_estimation":
            assert (float(out.sum_a[k]), float(out.sum_b[k])) == agg[key], key
            assert int(out.informative[k]) == pw[key].sites


def general_rows(rng, S, samples, half, with_missing):
    """Multi-allelic rows built to reach every branch of dense_collect_counts / _dense_dot / dense_hudson_sites_general: 3 to 8 distinct
    alleles met in a different first-seen order by the two populations, population 2 with fewer distinct alleles than population 1 and
    the reverse (and ties), biallelic rows among them; with missing calls also a missing entry at a population's first member, a
    population with one called haplotype (pi None) and one with none (dxy None).  Population 1 = columns [0, 2 half), population 2 =
    columns [2 half, 2 samples - 2) (the last sample in neither)."""
    Hc = 2 * samples
    c1, c2 = np.arange(0, 2 * half), np.arange(2 * half, Hc - 2)
    data = np.zeros((S, Hc), dtype=np.uint8)
    miss = np.zeros((S, Hc), dtype=bool)
    for r in range(S):
        kind = r % 8
        if kind == 0:    # biallelic row of a multi-allelic matrix: still the general formulas
            data[r] = rng.random(Hc) < rng.random()
            continue
        if kind == 7:    # anything
            data[r] = rng.integers(0, 8, size=Hc)
            continue
        k1 = int(rng.integers(3, 9)) if kind != 3 else int(rng.integers(1, 4))
        k2 = int(rng.integers(3, 9)) if kind != 4 else int(rng.integers(1, 4))
        if kind == 5:
            k2 = k1      # a tie: population 1 drives
        a1 = rng.permutation(8)[:k1]
        a2 = rng.permutation(8)[:k2]
        if kind == 6:
            a2 = a1[::-1].copy()  # the same alleles, met in the opposite order
        for cols, al in ((c1, a1), (c2, a2)):
            v = al[rng.integers(0, len(al), size=len(cols))]
            v[:len(al)] = al                      # every allele present, in the drawn first-seen order
            v[len(al):] = rng.permutation(v[len(al):])
            data[r, cols] = v
        data[r, Hc - 2:] = rng.integers(0, 8, size=2)
    if with_missing:
        miss |= rng.random((S, Hc)) < 0.05
        for r in range(1, S, 5):
            miss[r, c1[0]] = True                  # population 1's first member is missing
        for r in range(2, S, 7):
            miss[r, c2[0]] = miss[r, c2[1]] = True  # population 2's first sample
        for r in range(3, S, 11):
            miss[r, c1[1:]] = True                 # one called haplotype in population 1: pi1 None
        for r in range(4, S, 13):
            miss[r, c2] = True                     # nothing called in population 2: dxy None
        miss[S - 1, c1] = True
        data[miss] = 0
    return data, (miss if with_missing else None)


@pytest.mark.parametrize("with_missing,threads", [(False, 1), (False, 4), (True, 1), (True, 4)])
def test_c_general_twin_matches_python_oracle(with_missing, threads):
    """fo_hudson_sweep_general_threaded (the reference's dense arm for a matrix declared multi-allelic) against dense_hudson_sites_general
    bit for bit on every track, called counts and the per-site gather exactly, the general arms' per-population totals and the per-site
    sums against the Python restatement."""
    S, samples = 480, 33
    half = 15
    rng = np.random.default_rng(31 + threads + 10 * with_missing)
    data, miss = general_rows(rng, S, samples, half, with_missing)
    words = None
    if miss is not None:
        bits = np.packbits(miss.reshape(-1), bitorder="little")
        words = np.frombuffer(np.concatenate([bits, np.zeros((-len(bits)) % 8, np.uint8)]).tobytes(), dtype="<u8").copy()
    m = R.DenseGenotypeMatrix(bytes(data.reshape(-1)), None if words is None else [int(w) for w in words], S, samples, 2, int(data.max()))
    assert m.max_allele == 7
    h1, h2 = H.haps_for_samples(range(0, half)), H.haps_for_samples(range(half, samples - 1))
    off1, off2 = R.dense_membership_offsets(m, h1), R.dense_membership_offsets(m, h2)
    out = D.hudson_sweep_general(data.reshape(-1), words, S, m.stride, off1, off2, threads)
    exp = R.dense_hudson_sites_general(m, [R.Variant(i, None) for i in range(S)], off1, off2)
    H.assert_bits_equal(out.fst, [H.opt(x.fst) for x in exp], "fst")
    H.assert_bits_equal(out.dxy, [H.opt(x.d_xy) for x in exp], "dxy")
    H.assert_bits_equal(out.pi1, [H.opt(x.pi_pop1) for x in exp], "pi1")
    H.assert_bits_equal(out.pi2, [H.opt(x.pi_pop2) for x in exp], "pi2")
    H.assert_bits_equal(out.num, [H.opt(x.num_component) for x in exp], "num")
    H.assert_bits_equal(out.den, [H.opt(x.den_component) for x in exp], "den")
    assert np.array_equal(out.called[0], np.array([x.n1_called for x in exp], dtype=np.uint32))
    assert np.array_equal(out.called[1], np.array([x.n2_called for x in exp], dtype=np.uint32))
    # the edges the rows were built for are there
    assert any(x.pi_pop1 is None and x.n1_called == 1 for x in exp) == with_missing
    assert any(x.d_xy is None for x in exp) == with_missing
    assert any(x.fst is not None for x in exp)
    for p, (hl, off) in enumerate(((h1, off1), (h2, off2))):
        s = R.build_dense_population_summary(m, hl)
        assert np.array_equal(out.alt[p], np.array(s.alt_counts, dtype=np.uint32))
        assert np.array_equal(out.called[p], np.array(s.called_counts, dtype=np.uint32))
        pis = [x.pi_pop1 if p == 0 else x.pi_pop2 for x in exp]
        assert out.pop[p]["segregating_sites"] == R.count_segregating_sites_dense(m, off)
        assert out.pop[p]["uncallable_sites"] == sum(1 for v in pis if v is None)
        assert out.pop[p]["haplotype_capacity"] == len(off)
        assert H.rel_close(out.pop[p]["pi_sum"], sum(v for v in pis if v is not None), 1e-12)
        L = 10 * S
        assert H.rel_close(out.pop[p]["pi_sum"] / (L - out.pop[p]["uncallable_sites"]), R.calculate_pi_dense(m, off, L), 1e-12)
    ns, ds = R.hudson_component_sums(exp)
    assert H.rel_close(out.totals["site_num_sum"], ns, 1e-12) and H.rel_close(out.totals["site_den_sum"], ds, 1e-12)
    assert out.totals["sites_with_components"] == sum(1 for x in exp if x.num_component is not None)
    assert out.totals["site_dxy_skipped"] == sum(1 for x in exp if x.d_xy is None)
    L = 10 * S
    assert H.rel_close(out.totals["site_dxy_sum"] / (L - out.totals["site_dxy_skipped"]), R.calculate_dxy_dense(m, off1, off2, L), 1e-12)
    # dense_hudson_sites picks this arm by the declared max_allele, also for a matrix whose rows happen to be biallelic
    bi = (rng.random((50, 2 * samples)) < 0.4).astype(np.uint8)
    mb = R.DenseGenotypeMatrix(bytes(bi.reshape(-1)), None, 50, samples, 2, 3)
    eb = R.dense_hudson_sites(mb, [R.Variant(i, None) for i in range(50)], off1, off2)
    ob = D.hudson_sweep_dense(bi.reshape(-1), None, 50, mb.stride, mb.max_allele, off1, off2, threads)
    H.assert_bits_equal(ob.dxy, [H.opt(x.d_xy) for x in eb], "dxy, biallelic rows declared multi-allelic")
    H.assert_bits_equal(ob.pi1, [H.opt(x.pi_pop1) for x in eb], "pi1, biallelic rows declared multi-allelic")


REGION_CASES = [
    # (sites, samples, max_allele, p_missing, p_haploid, all_missing_rows)
    (150, 20, 1, 0.0, 0.0, 0),     # nothing missing: a matrix without missing words (the DENSE summary's no-missing arm)
    (150, 21, 1, 0.15, 0.05, 2),
    (120, 33, 2, 0.1, 0.1, 1),
    (120, 26, 5, 0.08, 0.05, 1),
    (90, 9, 1, 0.45, 0.1, 0),      # few calls per group: many sites with n < 2 and without any call
]


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("sites,samples,max_allele,p_missing,p_haploid,dead", REGION_CASES)
def test_c_region_sweep_matches_python_oracle(sites, samples, max_allele, p_missing, p_haploid, dead, threads):
    """fo_region_sweep_threaded (what fmh_pair_region_sweep computes) against the sparse restatement: the six tracks of
    calculate_hudson_fst_per_site and both groups' calculate_per_site_diversity bit for bit, called / distinct / alt exactly, and the totals
    against calculate_pi / calculate_pi_dense / build_dense_population_summary, count_segregating_sites_for_haplotypes,
    hudson_component_sums, calculate_d_xy_hudson and aggregate_hudson_components_from_summaries - equal with one thread (the same additions
    in the same order), to 1e-12 with more (ranges added in range order)."""
    rng = random.Random(sites * 7 + samples + max_allele)
    variants = H.random_sparse_variants(rng, sites, samples, max_allele, p_missing, p_haploid, dead)
    for i, a in ((sites // 2, 0), (sites // 2 + 1, max_allele), (sites - 1, 1)):  # monomorphic for one allele in both groups: FST 0 / 0
        variants[i] = R.make_variant(variants[i].position, [None if g is None else [a] * len(g) for g in variants[i].genotypes])
    m = H.dense_from_variants(variants, samples)
    words = H.missing_words_np(m)
    if not words.any():
        words = None
    m = R.DenseGenotypeMatrix(m.data, None if words is None else m.missing, sites, samples, m.ploidy, m.max_allele)
    assert (words is None) == (p_missing == 0 and p_haploid == 0 and dead == 0)
    data = np.frombuffer(m.data, dtype=np.uint8)
    third = samples // 3
    h1 = H.haps_for_samples(range(0, third))
    h2 = H.haps_for_samples(range(third, 2 * third)) + [(2 * third, 0)]  # one half-sample
    off1, off2 = R.dense_membership_offsets(m, h1), R.dense_membership_offsets(m, h2)
    names = [f"s{i}" for i in range(samples)]
    L = variants[-1].position + 10
    p1 = R.PopulationContext(0, h1, variants, names, L)
    p2 = R.PopulationContext(1, h2, variants, names, L)
    region = R.QueryRegion(0, L)
    exp = R.calculate_hudson_fst_per_site(p1, p2, region)
    div = [R.calculate_per_site_diversity(variants, hl, region) for hl in (h1, h2)]
    mems = [R.HapMembership.build(samples, hl) for hl in (h1, h2)]
    distinct = [[R.compute_pi_metrics_fast(v, mem)[2] for v in variants] for mem in mems]
    rows = data.reshape(sites, m.stride)

    def same(a, b):
        return a == b if threads == 1 else H.rel_close(a, b, 1e-12)

    formulas = [D.FORMULA_SPARSE, D.FORMULA_DENSE] + ([D.FORMULA_SUMMARY] if m.max_allele <= 1 else [])
    base = None
    for summary_formula in formulas:
        out = D.region_sweep(data, words, sites, m.stride, m.max_allele, off1, off2, summary_formula, D.FORMULA_SPARSE, threads)
        H.assert_bits_equal(out.fst, [H.opt(x.fst) for x in exp], "fst")
        H.assert_bits_equal(out.dxy, [H.opt(x.d_xy) for x in exp], "dxy")
        H.assert_bits_equal(out.pi1, [H.opt(x.pi_pop1) for x in exp], "pi1")
        H.assert_bits_equal(out.pi2, [H.opt(x.pi_pop2) for x in exp], "pi2")
        H.assert_bits_equal(out.num, [H.opt(x.num_component) for x in exp], "num")
        H.assert_bits_equal(out.den, [H.opt(x.den_component) for x in exp], "den")
        assert np.array_equal(out.called[0], np.array([x.n1_called for x in exp], dtype=np.uint32))
        assert np.array_equal(out.called[1], np.array([x.n2_called for x in exp], dtype=np.uint32))
        for p, (hl, off) in enumerate(((h1, off1), (h2, off2))):
            H.assert_bits_equal(out.site_pi[p], [x.pi for x in div[p]], f"site pi group {p}")
            H.assert_bits_equal(out.site_theta[p], [x.watterson_theta for x in div[p]], f"site theta group {p}")
            assert np.array_equal(out.distinct[p], np.array(distinct[p], dtype=np.uint32)), p
            assert np.array_equal(out.alt[p], rows[:, off].sum(axis=1, dtype=np.uint32)), p  # data is 0 under a missing call
            unc = sum(1 for x in exp if (x.n1_called if p == 0 else x.n2_called) < 2)
            pop = out.pop[p]
            assert pop["haplotype_capacity"] == len(off)
            assert pop["uncallable_sites"] == unc
            assert pop["segregating_sites"] == R.count_segregating_sites_for_haplotypes(variants, hl)
            if summary_formula == D.FORMULA_SPARSE:
                assert same(pop["pi_sum"] / (L - unc), R.calculate_pi(variants, hl, L)), p
            elif summary_formula == D.FORMULA_DENSE:
                assert same(pop["pi_sum"] / (L - unc), R.calculate_pi_dense(m, off, L)), p
            else:
                assert same(pop["pi_sum"], R.build_dense_population_summary(m, hl).pi_sum), p
        t = out.totals
        ns, ds = R.hudson_component_sums(exp)
        assert same(t["site_num_sum"], ns) and same(t["site_den_sum"], ds)
        assert t["sites_with_components"] == sum(1 for x in exp if x.num_component is not None)
        assert t["site_dxy_skipped"] == sum(1 for x in exp if x.d_xy is None)
        assert same(t["site_dxy_sum"] / (L - t["site_dxy_skipped"]), R.calculate_d_xy_hudson(p1, p2))
        if m.max_allele <= 1:
            s = R.aggregate_hudson_components_from_summaries(R.build_dense_population_summary(m, h1), R.build_dense_population_summary(m, h2))
            for k in ("numerator_sum", "denominator_sum", "pi1_sum", "pi2_sum", "dxy_sum_all"):
                assert same(t[k], getattr(s, k)), k
            assert t["dxy_uncallable_sites"] == s.dxy_uncallable_sites
        base = out
    # the edges are there
    assert any(x.n1_called == 1 for x in exp) or p_missing < 0.3
    assert any(x.d_xy is None for x in exp) or (dead == 0 and p_missing < 0.3)
    assert any(x.num_component == 0.0 and x.den_component == 0.0 for x in exp)
    assert any(x.watterson_theta == 0.0 for x in div[0]) and any(x.watterson_theta > 0.0 for x in div[1])
    # without the Hudson part: no track, Hudson totals zero, the rest unchanged
    none = D.region_sweep(data, words, sites, m.stride, m.max_allele, off1, off2, formulas[-1], -1, threads)
    assert none.fst is None and all(v == 0 for v in none.totals.values())
    assert none.pop == base.pop
    for k in ("alt", "called", "distinct", "site_pi", "site_theta"):
        assert np.array_equal(getattr(none, k).view(np.uint64 if k.startswith("site") else np.uint32),
                              getattr(base, k).view(np.uint64 if k.startswith("site") else np.uint32)), k
    with pytest.raises(ValueError):
        D.region_sweep(data, words, sites, m.stride, m.max_allele, off1, off2, D.FORMULA_SPARSE, D.FORMULA_DENSE, threads)


# ---- fo_pairwise_differences_threaded: the bit-parallel all-pairs oracle of tests/test_gpu_scale_pairwise.py ----

PD_PLOIDIES = [1, 2, 3, 4, 5, 9]
PD_SITES = [1, 63, 64, 65, 200]   # around the 64-site word of the transpose
PD_MAX_ALLELES = [1, 2, 3, 7, 9]  # 1, 2, 2, 3 and 4 allele bits
PD_MISSING = [0.0, 0.05, 0.5]
PD_SAMPLES = [2, 40, 7, 23, 31, 12]


def _pd_case_data(case):
    """(max_allele, missing fraction) of case = ploidy index p + 6 x site-count index q: allele range (p + q) % 5, missing fraction
    (p + 2 q) % 3.  Every pair of {ploidy, site count, allele range, missing fraction} then meets all of its combinations
    (test_c_pairwise_parameter_coverage)."""
    p, q = case % len(PD_PLOIDIES), case // len(PD_PLOIDIES)
    return PD_MAX_ALLELES[(p + q) % len(PD_MAX_ALLELES)], PD_MISSING[(p + 2 * q) % len(PD_MISSING)]


def _pd_cohort(rng, sites, samples, ploidy, max_allele, p_missing):
    """Random u8 matrix [sites][samples * ploidy] + missing words, and the same cohort as the reference's variants: every genotype the
    prefix of its called alleles (CompressedGenotypes::get), None when the prefix is empty."""
    Hc = samples * ploidy
    data = rng.integers(0, max_allele + 1, size=(sites, Hc), dtype=np.uint8)
    data[rng.random((sites, Hc)) < 0.4] = 0
    miss = rng.random((sites, Hc)) < p_missing if p_missing > 0 else np.zeros((sites, Hc), dtype=bool)
    data[miss] = 0
    words = None
    if p_missing > 0:
        bits = np.packbits(miss.reshape(-1), bitorder="little")
        words = np.frombuffer(np.concatenate([bits, np.zeros((-len(bits)) % 8, np.uint8)]).tobytes(), dtype="<u8").copy()
    variants = []
    for s in range(sites):
        row = []
        for i in range(samples):
            g = []
            for k in range(ploidy):
                if miss[s, i * ploidy + k]:
                    break
                g.append(int(data[s, i * ploidy + k]))
            row.append(g or None)
        variants.append(R.make_variant(s + 1, row))
    return data, words, variants


def _pd_check_against_reference(data, words, variants, sites, samples, ploidy, max_allele, n, threads):
    diff, both = D.pairwise_differences(data, words, sites, samples * ploidy, ploidy, n, max_allele, threads)
    L = sites + 3  # sequence_length >= sites: `comparable` never clamps at 0
    ref = R.calculate_pairwise_differences(variants, n, L)
    assert len(ref) == n * (n - 1) // 2
    first_len = [next((len(v.genotypes.get(i)) for v in variants if v.genotypes.get(i) is not None), 0) for i in range(n)]
    for (i, j), d, comparable in ref:
        assert int(diff[i, j]) == d, (i, j)
        hi, hj = first_len[i], first_len[j]
        if hi == 0 or hj == 0:  # a sample that is never called: the reference reports (0, 0)
            assert int(both[i, j]) == 0 and comparable == 0
            continue
        lost = L * hi * hj - comparable
        assert lost % (hi * hj) == 0
        assert int(both[i, j]) == sites - lost // (hi * hj), (i, j)
    assert not np.tril(diff).any() and not np.tril(both).any()
    return diff, both


@pytest.mark.parametrize("case", range(len(PD_PLOIDIES) * len(PD_SITES)))
def test_c_pairwise_matches_python_oracle(case):
    """diff equal to calculate_pairwise_differences (stats.rs:4106-4231) pair by pair, both recovered from its comparable-site count;
    one thread and several threads give the same arrays."""
    ploidy, sites = PD_PLOIDIES[case % len(PD_PLOIDIES)], PD_SITES[case // len(PD_PLOIDIES)]
    max_allele, p_missing = _pd_case_data(case)
    samples = PD_SAMPLES[(case + case // 6) % len(PD_SAMPLES)]
    if ploidy >= 5 and sites == 200:
        samples = min(samples, 12)  # the Python reference walks ploidy^2 allele pairs per site and sample pair
    rng = np.random.default_rng(4106 + case)
    data, words, variants = _pd_cohort(rng, sites, samples, ploidy, max_allele, p_missing)
    diff, both = _pd_check_against_reference(data, words, variants, sites, samples, ploidy, max_allele, samples, 1)
    for threads in (3, 16):
        d2, b2 = D.pairwise_differences(data, words, sites, samples * ploidy, ploidy, samples, max_allele, threads)
        assert np.array_equal(d2, diff) and np.array_equal(b2, both)


def test_c_pairwise_parameter_coverage():
    """The case table above meets every value the pin asks for, every (ploidy, missing fraction), every (max_allele, missing fraction) and
    every (ploidy, max_allele) combination."""
    cases = range(len(PD_PLOIDIES) * len(PD_SITES))
    rows = [(PD_PLOIDIES[c % len(PD_PLOIDIES)],) + _pd_case_data(c) for c in cases]
    assert {(p, m) for p, _, m in rows} == {(p, m) for p in PD_PLOIDIES for m in PD_MISSING}
    assert {(a, m) for _, a, m in rows} == {(a, m) for a in PD_MAX_ALLELES for m in PD_MISSING}
    assert {(p, a) for p, a, _ in rows} == {(p, a) for p in PD_PLOIDIES for a in PD_MAX_ALLELES}
    sites = [PD_SITES[c // len(PD_PLOIDIES)] for c in cases]
    assert {(s, r[1]) for s, r in zip(sites, rows)} == {(s, a) for s in PD_SITES for a in PD_MAX_ALLELES}
    assert {(s, r[2]) for s, r in zip(sites, rows)} == {(s, m) for s in PD_SITES for m in PD_MISSING}
    assert {PD_SAMPLES[(c + c // 6) % len(PD_SAMPLES)] for c in cases} >= {2, 40}


@pytest.mark.parametrize("max_allele", [1, 3, 5])
@pytest.mark.parametrize("p_missing", [0.05, 0.5])
def test_c_pairwise_diploid_with_missing_slots(max_allele, p_missing):
    """Ploidy 2 with calls missing slot by slot - (called, missing) is a haploid genotype, (missing, called) is None: the prefix rule the
    full-size general cohorts of tests/test_gpu_scale_pairwise.py rest on."""
    sites, samples = 150, 24
    data, words, variants = _pd_cohort(np.random.default_rng(int(p_missing * 100) + max_allele), sites, samples, 2, max_allele, p_missing)
    lengths = {len(g) for v in variants for g in (v.genotypes.get(i) for i in range(samples)) if g is not None}
    assert lengths == {1, 2} and any(v.genotypes.get(i) is None for v in variants for i in range(samples))
    _pd_check_against_reference(data, words, variants, sites, samples, 2, max_allele, samples, 3)


@pytest.mark.parametrize("ploidy,max_allele,p_missing", [(2, 1, 0.0), (3, 5, 0.1), (1, 9, 0.3)])
def test_c_pairwise_sample_subset(ploidy, max_allele, p_missing):
    """n_samples < samples: the first n samples of wider rows (the stride stays the matrix's)."""
    sites, samples = 130, 19
    data, words, variants = _pd_cohort(np.random.default_rng(ploidy * 100 + max_allele), sites, samples, ploidy, max_allele, p_missing)
    full, full_both = D.pairwise_differences(data, words, sites, samples * ploidy, ploidy, samples, max_allele, 2)
    for n in (2, 7, samples - 1):
        diff, both = _pd_check_against_reference(data, words, variants, sites, samples, ploidy, max_allele, n, 4)
        assert np.array_equal(diff, full[:n, :n]) and np.array_equal(both, full_both[:n, :n])


def test_c_pairwise_reference_literal_cases(kats):
    """src/tests/stats_tests.rs:368-470 (the four tests behind kats['pairwise_differences']) through the C oracle: diff per pair, and
    the comparable-site count rebuilt from `both` the way the reference counts it."""
    n_expected = 0
    for case in kats["pairwise_differences"]["cases"]:
        n, L, sites = case["sample_count"], case["sequence_length"], len(case["variants"])
        ploidy = max(len(g) for _, genos in case["variants"] for g in genos if g is not None)
        data = np.zeros((sites, n * ploidy), dtype=np.uint8)
        miss = np.zeros((sites, n * ploidy), dtype=bool)
        for s, (_, genos) in enumerate(case["variants"]):
            for i, g in enumerate(genos):
                g = g or []
                data[s, i * ploidy:i * ploidy + len(g)] = g
                miss[s, i * ploidy + len(g):(i + 1) * ploidy] = True
        bits = np.packbits(miss.reshape(-1), bitorder="little")
        words = np.frombuffer(np.concatenate([bits, np.zeros((-len(bits)) % 8, np.uint8)]).tobytes(), dtype="<u8").copy()
        diff, both = D.pairwise_differences(data, words if miss.any() else None, sites, n * ploidy, ploidy, n, int(data.max()), 2)
        for key, (exp_diff, exp_comparable) in case["expected"].items():
            i, j = (int(x) for x in key.split(","))
            assert int(diff[i, j]) == exp_diff, (case["name"], key)
            assert (L - (sites - int(both[i, j]))) * ploidy * ploidy == exp_comparable, (case["name"], key)
            n_expected += 1
    assert n_expected == 5
