"""ctypes wrapper of oracle/liboracle_dense.so (the C half of the CPU oracle).

TEST INFRASTRUCTURE ONLY — see the header of oracle/dense_oracle.c.  Imported by tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg, never by the product."""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FERROMIC_ORACLE_LIB") or os.path.join(_HERE, "liboracle_dense.so")  # the override: the sanitizer build (oracle/Makefile asan)


class PopTotals(C.Structure):
    _fields_ = [("haplotype_capacity", C.c_uint64), ("segregating_sites", C.c_uint64),
                ("uncallable_sites", C.c_uint64), ("pi_sum", C.c_double)]


class HudsonTotals(C.Structure):
    _fields_ = [("numerator_sum", C.c_double), ("denominator_sum", C.c_double), ("pi1_sum", C.c_double),
                ("pi2_sum", C.c_double), ("dxy_sum_all", C.c_double), ("dxy_uncallable_sites", C.c_uint64),
                ("site_num_sum", C.c_double), ("site_den_sum", C.c_double), ("sites_with_components", C.c_uint64)]


class HudsonGeneralTotals(C.Structure):
    _fields_ = [("site_num_sum", C.c_double), ("site_den_sum", C.c_double), ("site_dxy_sum", C.c_double),
                ("sites_with_components", C.c_uint64), ("site_dxy_skipped", C.c_uint64)]


class RegionTotals(C.Structure):  # the Hudson fields of fmh_hudson_totals
    _fields_ = HudsonTotals._fields_ + [("site_dxy_sum", C.c_double), ("site_dxy_skipped", C.c_uint64)]


FORMULA_SPARSE, FORMULA_DENSE, FORMULA_SUMMARY = 0, 1, 2  # FMH_FORMULA_*

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            subprocess.run(["make", "-C", _HERE], check=True)
        lib = C.CDLL(LIB_PATH)
        vp, sz, u64, u32, i = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int
        lib.fo_generate.argtypes = [vp, vp, sz, sz, u64, u64, vp, vp, u32, i]
        lib.fo_generate.restype = None
        lib.fo_hudson_sweep_threaded.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz] + [vp] * 10 + [
            C.POINTER(PopTotals), C.POINTER(HudsonTotals), i]
        lib.fo_hudson_sweep_threaded.restype = None
        lib.fo_hudson_sweep_general_threaded.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz] + [vp] * 10 + [
            C.POINTER(PopTotals), C.POINTER(HudsonGeneralTotals), i]
        lib.fo_hudson_sweep_general_threaded.restype = None
        lib.fo_wc_sites_threaded.argtypes = [vp, vp, sz, sz, vp, i, vp, vp, vp, vp, vp, vp, i]
        lib.fo_wc_sites_threaded.restype = None
        lib.fo_region_sweep_threaded.argtypes = [vp, vp, sz, sz, i, vp, sz, vp, sz, i, i] + [vp] * 11 + [
            C.POINTER(PopTotals), C.POINTER(RegionTotals), i]
        lib.fo_region_sweep_threaded.restype = i
        lib.fo_pairwise_differences_threaded.argtypes = [vp, vp, sz, sz, sz, sz, i, vp, vp, i]
        lib.fo_pairwise_differences_threaded.restype = i
        _lib = lib
    return _lib


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def generate(variants: int, columns: int, seed: int, first_site: int, thresholds24: np.ndarray,
             pop_of_column: np.ndarray, missing_threshold24: int = 0, nthreads: int = 1):
    """Host-layout matrix (and missing words) of the counter-based synthetic cohort."""
    thr = np.ascontiguousarray(thresholds24, dtype=np.uint32)
    poc = np.ascontiguousarray(pop_of_column, dtype=np.uint8)
    assert thr.shape[1] == variants and poc.size == columns
    data = np.empty(variants * columns, dtype=np.uint8)
    words = np.zeros((variants * columns + 63) // 64, dtype=np.uint64) if missing_threshold24 else None
    load().fo_generate(_p(data), _p(words), variants, columns, seed, first_site, _p(thr), _p(poc),
                       missing_threshold24, nthreads)
    return data, words


@dataclass
class SweepOut:
    alt: np.ndarray      # [2][S] u32
    called: np.ndarray   # [2][S]
    fst: Optional[np.ndarray]
    dxy: Optional[np.ndarray]
    pi1: Optional[np.ndarray]
    pi2: Optional[np.ndarray]
    num: Optional[np.ndarray]
    den: Optional[np.ndarray]
    pop: list
    totals: dict


def hudson_sweep(data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, stride: int,
                 offsets1: np.ndarray, offsets2: np.ndarray, nthreads: int = 1, want_sites: bool = True) -> SweepOut:
    """fo_hudson_sweep_threaded: summaries x2 + Hudson totals + per-site records (biallelic dense)."""
    o1 = np.ascontiguousarray(offsets1, dtype=np.uint64)
    o2 = np.ascontiguousarray(offsets2, dtype=np.uint64)
    alt = np.empty((2, variants), dtype=np.uint32)
    called = np.empty((2, variants), dtype=np.uint32)
    tracks = [np.empty(variants, dtype=np.float64) if want_sites else None for _ in range(6)]
    pop = (PopTotals * 2)()
    tot = HudsonTotals()
    load().fo_hudson_sweep_threaded(_p(data), _p(missing_words), variants, stride, _p(o1), o1.size, _p(o2), o2.size,
                                    _p(alt[0]), _p(called[0]), _p(alt[1]), _p(called[1]),
                                    *[_p(t) for t in tracks], pop, C.byref(tot), nthreads)
    return SweepOut(alt, called, *tracks,
                    pop=[{k: getattr(pop[i], k) for k, _ in PopTotals._fields_} for i in range(2)],
                    totals={k: getattr(tot, k) for k, _ in HudsonTotals._fields_})


def hudson_sweep_general(data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, stride: int,
                         offsets1: np.ndarray, offsets2: np.ndarray, nthreads: int = 1, want_sites: bool = True) -> SweepOut:
    """fo_hudson_sweep_general_threaded: dense_hudson_sites_general (the reference's arm for every row of a matrix declared with
    max_allele > 1) per site, the general arms' per-population totals (segregating = a second allele among the called entries,
    uncallable = fewer than two calls, pi_sum) and the per-site sums (site_num_sum, site_den_sum, sites_with_components,
    site_dxy_sum, site_dxy_skipped).  alt / called: build_dense_population_summary's gather (alt = sum of the allele values)."""
    o1 = np.ascontiguousarray(offsets1, dtype=np.uint64)
    o2 = np.ascontiguousarray(offsets2, dtype=np.uint64)
    alt = np.empty((2, variants), dtype=np.uint32)
    called = np.empty((2, variants), dtype=np.uint32)
    tracks = [np.empty(variants, dtype=np.float64) if want_sites else None for _ in range(6)]
    pop = (PopTotals * 2)()
    tot = HudsonGeneralTotals()
    load().fo_hudson_sweep_general_threaded(_p(data), _p(missing_words), variants, stride, _p(o1), o1.size, _p(o2), o2.size,
                                            _p(alt[0]), _p(called[0]), _p(alt[1]), _p(called[1]),
                                            *[_p(t) for t in tracks], pop, C.byref(tot), nthreads)
    return SweepOut(alt, called, *tracks,
                    pop=[{k: getattr(pop[i], k) for k, _ in PopTotals._fields_} for i in range(2)],
                    totals={k: getattr(tot, k) for k, _ in HudsonGeneralTotals._fields_})


def hudson_sweep_dense(data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, stride: int, max_allele: int,
                       offsets1: np.ndarray, offsets2: np.ndarray, nthreads: int = 1, want_sites: bool = True) -> SweepOut:
    """dense_hudson_sites' choice (stats.rs:3060-3070): the biallelic sweep for a matrix declared max_allele <= 1, else the general twin."""
    f = hudson_sweep if max_allele <= 1 else hudson_sweep_general
    return f(data, missing_words, variants, stride, offsets1, offsets2, nthreads, want_sites)


@dataclass
class WcOut:
    a: Optional[np.ndarray]       # [slots][S]; slot 0 = overall, then pairs (0,1), (0,2), ...  (None: sites=False)
    b: Optional[np.ndarray]
    state: Optional[np.ndarray]   # 0 calculable, 1 indeterminate, 2 no variance, 3 insufficient
    sum_a: np.ndarray
    sum_b: np.ndarray
    informative: np.ndarray


def wc_sites(data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, stride: int, group_of_column: np.ndarray,
             n_groups: int, nthreads: int = 1, sites: bool = True) -> WcOut:
    """fo_wc_sites_threaded: Weir & Cockerham per site + regional sums (stats.rs:1814-2032, 2145-2374) on a dense matrix.
    sites=False: no per-site arrays, only the regional sums and informative counts (each thread's range summed in site order, the
    ranges added in order: nthreads=1 gives the reference's serial sums)."""
    goc = np.ascontiguousarray(group_of_column, dtype=np.uint8)
    assert goc.size == stride and 2 <= n_groups <= 32
    slots = 1 + n_groups * (n_groups - 1) // 2
    a = np.empty((slots, variants), dtype=np.float64) if sites else None
    b = np.empty((slots, variants), dtype=np.float64) if sites else None
    st = np.empty((slots, variants), dtype=np.uint8) if sites else None
    sa, sb, inf = np.zeros(slots), np.zeros(slots), np.zeros(slots, dtype=np.uint64)
    load().fo_wc_sites_threaded(_p(data), _p(missing_words), variants, stride, _p(goc), n_groups, _p(a), _p(b), _p(st), _p(sa), _p(sb),
                                _p(inf), nthreads)
    return WcOut(a, b, st, sa, sb, inf)


@dataclass
class RegionOut:
    alt: np.ndarray         # [2][S] u32: the sum of the allele values (hudson_sweep's gather)
    called: np.ndarray      # [2][S] u32
    distinct: np.ndarray    # [2][S] u32
    site_pi: np.ndarray     # [2][S] f64: calculate_per_site_diversity of each group
    site_theta: np.ndarray  # [2][S]
    fst: Optional[np.ndarray]
    dxy: Optional[np.ndarray]
    pi1: Optional[np.ndarray]
    pi2: Optional[np.ndarray]
    num: Optional[np.ndarray]
    den: Optional[np.ndarray]
    pop: list
    totals: dict


def region_sweep(data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, stride: int, max_allele: int,
                 offsets1: np.ndarray, offsets2: np.ndarray, summary_formula: int, hudson_formula: int = FORMULA_SPARSE,
                 nthreads: int = 1) -> RegionOut:
    """fo_region_sweep_threaded: what fmh_pair_region_sweep computes - per site and group called / distinct / alt and the per-site
    diversity (pi, theta), the six sparse Hudson tracks (hudson_formula = FORMULA_SPARSE; None below 0), the population totals by
    summary_formula (SPARSE, DENSE: its no-missing biallelic arm when missing_words is None and max_allele <= 1, SUMMARY) and the Hudson
    fields of fmh_hudson_totals.  Tracks are NaN where the reference has None."""
    o1 = np.ascontiguousarray(offsets1, dtype=np.uint64)
    o2 = np.ascontiguousarray(offsets2, dtype=np.uint64)
    if missing_words is not None:
        missing_words = np.ascontiguousarray(missing_words, dtype=np.uint64)
    counts = [np.empty((2, variants), dtype=np.uint32) for _ in range(3)]
    div = [np.empty((2, variants), dtype=np.float64) for _ in range(2)]
    tracks = [np.empty(variants, dtype=np.float64) if hudson_formula >= 0 else None for _ in range(6)]
    pop = (PopTotals * 2)()
    tot = RegionTotals()
    rc = load().fo_region_sweep_threaded(_p(np.ascontiguousarray(data, dtype=np.uint8)), _p(missing_words), variants, stride, int(max_allele),
                                         _p(o1), o1.size, _p(o2), o2.size, int(summary_formula), int(hudson_formula),
                                         *[_p(a) for a in counts + div + tracks], pop, C.byref(tot), nthreads)
    if rc != 0:
        raise ValueError(f"formulas outside the model: summary {summary_formula}, Hudson {hudson_formula}")
    return RegionOut(*counts, *div, *tracks,
                     pop=[{k: getattr(pop[i], k) for k, _ in PopTotals._fields_} for i in range(2)],
                     totals={k: getattr(tot, k) for k, _ in RegionTotals._fields_})


def pairwise_differences(data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, stride: int, ploidy: int, n_samples: int,
                         max_allele: int, nthreads: int = 1):
    """fo_pairwise_differences_threaded: (diff, both) as [n_samples, n_samples] uint64 arrays, upper triangle filled, of the first
    n_samples samples of a site-major u8 matrix [variants][stride] (stride >= n_samples * ploidy columns, missing bit = site * stride +
    column): calculate_pairwise_differences (stats.rs:4106-4231) with every genotype the prefix of its called alleles, computed
    bit-parallel on haplotypes (XOR + popcount), not from allele counts."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    assert data.size >= variants * stride and n_samples * ploidy <= stride
    if missing_words is not None:
        missing_words = np.ascontiguousarray(missing_words, dtype=np.uint64)
        assert missing_words.size >= (variants * stride + 63) // 64
    diff = np.empty((n_samples, n_samples), dtype=np.uint64)
    both = np.empty((n_samples, n_samples), dtype=np.uint64)
    rc = load().fo_pairwise_differences_threaded(_p(data), _p(missing_words), variants, stride, ploidy, n_samples, int(max_allele),
                                                 _p(diff), _p(both), int(nthreads))
    if rc != 0:
        raise MemoryError("fo_pairwise_differences_threaded: the haplotype-major transpose does not fit in memory")
    return diff, both
