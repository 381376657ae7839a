"""Thin object layer over the C-ABI: device matrices, memberships and sweeps returning numpy.

Everything here runs on the GPU through libferromic_hip.so.  Host work is limited to building
masks and reshaping outputs.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _abi
from ._abi import FORMULA_DENSE, FORMULA_SPARSE, FORMULA_SUMMARY, WC_STATES  # noqa: F401


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class DeviceBuffer:
    """A hipMalloc'd buffer freed with the object."""

    def __init__(self, device: int, nbytes: int):
        self.device = device
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _abi.check(_abi.load().fmh_device_alloc(device, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def to_numpy(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if count:
            _abi.check(_abi.load().fmh_copy_to_host(self.device, _ptr(out), self.ptr, out.nbytes, None))
        return out

    @classmethod
    def from_numpy(cls, device: int, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        buf = cls(device, max(a.nbytes, 1))
        if a.nbytes:
            _abi.check(_abi.load().fmh_copy_to_device(device, buf.ptr, _ptr(a), a.nbytes, None))
        return buf

    def free(self):
        if getattr(self, "ptr", None):
            _abi.load().fmh_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceMatrix:
    """fmh_matrix handle == DenseGenotypeMatrix (stats.rs:250-331) resident in HBM."""

    def __init__(self, handle: int):
        self._h = handle
        lib = _abi.load()
        v, s, p, pitch, bp = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        hm, ma, dev = C.c_int(), C.c_uint8(), C.c_int()
        _abi.check(lib.fmh_matrix_info(handle, C.byref(v), C.byref(s), C.byref(p), C.byref(pitch), C.byref(bp),
                                       C.byref(hm), C.byref(ma), C.byref(dev)))
        self.variants, self.samples, self.ploidy = v.value, s.value, p.value
        self.pitch, self.bits_pitch = pitch.value, bp.value
        self.has_missing, self.max_allele, self.device = bool(hm.value), ma.value, dev.value
        self.columns = self.samples * self.ploidy

    @classmethod
    def from_host(cls, data: np.ndarray, missing_words: Optional[np.ndarray], variants: int, samples: int,
                  ploidy: int, max_allele: int, device: int = 0) -> "DeviceMatrix":
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        if data.size != variants * samples * ploidy:
            raise ValueError("dense genotype matrix requires variants * samples * ploidy entries")
        if missing_words is not None:
            missing_words = np.ascontiguousarray(missing_words, dtype=np.uint64)
        h = C.c_void_p()
        _abi.check(_abi.load().fmh_matrix_create(_ptr(data), _ptr(missing_words), variants, samples, ploidy,
                                                 int(max_allele), device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_host_planes(cls, planes: Sequence[np.ndarray], called: Optional[np.ndarray], variants: int, samples: int, ploidy: int,
                         max_allele: int, device: int = 0) -> "DeviceMatrix":
        """fmh_matrix_create_packed: host bit planes [variants][pitch] uint8 (column c = bit c & 7 of byte c >> 3), plane k = bit k of
        the allele value; `called` the same shape with 1 bits for called entries, or None."""
        planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
        pitch = planes[0].shape[1] if variants else 0
        ptrs = [_ptr(p) for p in planes] + [None] * (3 - len(planes))
        if called is not None:
            called = np.ascontiguousarray(called, dtype=np.uint8)
        h = C.c_void_p()
        _abi.check(_abi.load().fmh_matrix_create_packed(ptrs[0], ptrs[1], ptrs[2], _ptr(called), pitch, variants, samples, ploidy,
                                                        int(max_allele), device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def alloc(cls, variants: int, samples: int, ploidy: int, with_missing: bool, max_allele: int = 1,
              device: int = 0) -> "DeviceMatrix":
        h = C.c_void_p()
        _abi.check(_abi.load().fmh_matrix_alloc(variants, samples, ploidy, int(with_missing), max_allele, device,
                                                C.byref(h)))
        return cls(h.value)

    @classmethod
    def wrap(cls, d_data: int, pitch: int, d_bits: Optional[int], bits_pitch: int, variants: int, samples: int,
             ploidy: int, max_allele: int, device: int = 0) -> "DeviceMatrix":
        h = C.c_void_p()
        _abi.check(_abi.load().fmh_matrix_wrap(d_data, pitch, d_bits, bits_pitch, variants, samples, ploidy,
                                               max_allele, device, C.byref(h)))
        return cls(h.value)

    def generate(self, seed: int, first_global_site: int, thresholds24: np.ndarray, pop_of_column: np.ndarray,
                 missing_threshold24: int = 0) -> None:
        thr = np.ascontiguousarray(thresholds24, dtype=np.uint32)
        poc = np.ascontiguousarray(pop_of_column, dtype=np.uint8)
        if thr.ndim != 2 or thr.shape[1] != self.variants or poc.size != self.columns:
            raise ValueError("thresholds must be [n_pops][variants] and pop_of_column [columns]")
        _abi.check(_abi.load().fmh_matrix_generate(self._h, seed, first_global_site, _ptr(thr), _ptr(poc),
                                                   thr.shape[0], missing_threshold24, None))
        self.max_allele = max(self.max_allele, 1)

    def pack(self, release_bytes: bool = False) -> None:
        """fmh_matrix_pack: build the bit-packed image the sweeps prefer (alleles 0..3); optionally drop the u8 rows."""
        _abi.check(_abi.load().fmh_matrix_pack(self._h, 1 if release_bytes else 0))

    def download(self):
        data = np.empty(self.variants * self.columns, dtype=np.uint8)
        words = None
        if self.has_missing:
            words = np.zeros((self.variants * self.columns + 63) // 64, dtype=np.uint64)
        _abi.check(_abi.load().fmh_matrix_download(self._h, _ptr(data), _ptr(words)))
        return data, words

    def scan_max_allele(self) -> int:
        out = C.c_uint8()
        _abi.check(_abi.load().fmh_matrix_scan_max_allele(self._h, C.byref(out), None))
        return out.value

    def close(self):
        if getattr(self, "_h", None):
            _abi.load().fmh_matrix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Groups:
    """fmh_groups handle: P column memberships as 0/1 masks."""

    def __init__(self, matrix: DeviceMatrix, masks: np.ndarray):
        masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if masks.ndim != 2 or masks.shape[1] != matrix.columns:
            raise ValueError("masks must be [n_groups][samples*ploidy]")
        self.matrix = matrix
        self.n_groups = masks.shape[0]
        self.sizes = [int(x) for x in masks.astype(bool).sum(axis=1)]
        h = C.c_void_p()
        _abi.check(_abi.load().fmh_groups_create(matrix._h, _ptr(masks), self.n_groups, C.byref(h)))
        self._h = h.value

    @staticmethod
    def mask_from_haplotypes(matrix: DeviceMatrix, haplotypes: Sequence) -> np.ndarray:
        """DenseMembership::build (stats.rs:1252-1284) / HapMembership::build (1212-1238) as a column
        mask: duplicates collapse, out-of-range samples are skipped, Right is skipped if ploidy <= 1."""
        mask = np.zeros(matrix.columns, dtype=np.uint8)
        for sample_idx, side in haplotypes:
            if sample_idx >= matrix.samples:
                continue
            if side == 0:
                mask[sample_idx * matrix.ploidy] = 1
            else:
                if matrix.ploidy <= 1:
                    continue
                mask[sample_idx * matrix.ploidy + 1] = 1
        return mask

    @classmethod
    def from_haplotype_lists(cls, matrix: DeviceMatrix, lists: Sequence[Sequence]) -> "Groups":
        return cls(matrix, np.stack([cls.mask_from_haplotypes(matrix, hl) for hl in lists]))

    def close(self):
        if getattr(self, "_h", None):
            _abi.load().fmh_groups_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SWEEP_SUMMARY, SWEEP_HUDSON, SWEEP_DIVERSITY, SWEEP_REGION, SWEEP_WC = 1, 3, 5, 7, 8  # FMH_SWEEP_* of include/ferromic_hip.h


def sweep_window(m: DeviceMatrix, g: Groups, mode: int):
    """fmh_sweep_window: (first vector, vectors, derived group or -1) - what the next sweep of `mode` reads of every row."""
    first, count, derived = C.c_uint32(), C.c_uint32(), C.c_int()
    _abi.check(_abi.load().fmh_sweep_window(m._h, g._h, mode, C.byref(first), C.byref(count), C.byref(derived)))
    return first.value, count.value, derived.value


def sweep_tiled(m: DeviceMatrix, g: Groups, mode: int):
    """fmh_sweep_tiled: (whether the next sweep of `mode` reads the tile-transposed plane image, that image's bytes or 0)."""
    tiled, image_bytes = C.c_int(), C.c_size_t()
    _abi.check(_abi.load().fmh_sweep_tiled(m._h, g._h, mode, C.byref(tiled), C.byref(image_bytes)))
    return bool(tiled.value), image_bytes.value


def sweep_prefix(m: DeviceMatrix, g: Groups, mode: int):
    """fmh_sweep_prefix: (whether the next sweep of `mode` answers its counted groups from the prefix counts, the plane vectors per row it
    still reads, the table's bytes or 0)."""
    uses, vecs, table_bytes = C.c_int(), C.c_uint32(), C.c_size_t()
    _abi.check(_abi.load().fmh_sweep_prefix(m._h, g._h, mode, C.byref(uses), C.byref(vecs), C.byref(table_bytes)))
    return bool(uses.value), vecs.value, table_bytes.value


def _pop_totals(t: _abi.PopTotals) -> Dict[str, float]:
    return dict(haplotype_capacity=int(t.haplotype_capacity), segregating_sites=int(t.segregating_sites),
                uncallable_sites=int(t.uncallable_sites), pi_sum=float(t.pi_sum))


@dataclass
class SummaryResult:
    totals: List[Dict[str, float]]
    alt: Optional[np.ndarray]  # [P][rows] u32
    called: Optional[np.ndarray]


def population_summaries(m: DeviceMatrix, g: Groups, formula: int = FORMULA_SUMMARY, row_begin: int = 0,
                         row_count: Optional[int] = None, want_sites: bool = True, stream=None) -> SummaryResult:
    rows = m.variants - row_begin if row_count is None else row_count
    P = g.n_groups
    d_alt = DeviceBuffer(m.device, 4 * P * rows) if want_sites else None
    d_called = DeviceBuffer(m.device, 4 * P * rows) if want_sites else None
    totals = (_abi.PopTotals * P)()
    _abi.check(_abi.load().fmh_population_summaries(m._h, g._h, row_begin, rows, formula,
                                                    d_alt.ptr if d_alt else None, d_called.ptr if d_called else None,
                                                    totals, stream))
    alt = d_alt.to_numpy(np.uint32, P * rows).reshape(P, rows) if want_sites else None
    called = d_called.to_numpy(np.uint32, P * rows).reshape(P, rows) if want_sites else None
    return SummaryResult([_pop_totals(totals[p]) for p in range(P)], alt, called)


@dataclass
class HudsonResult:
    totals: Dict[str, float]
    pop: List[Dict[str, float]]
    sites: Optional[Dict[str, np.ndarray]]


def hudson_totals_dict(t: _abi.HudsonTotals) -> Dict[str, float]:
    return {k: (float(getattr(t, k)) if isinstance(getattr(t, k), float) else int(getattr(t, k)))
            for k, _ in _abi.HudsonTotals._fields_ if k != "pop"}


def hudson_sweep(m: DeviceMatrix, g: Groups, formula: int, row_begin: int = 0, row_count: Optional[int] = None,
                 want_sites: bool = True, stream=None) -> HudsonResult:
    rows = m.variants - row_begin if row_count is None else row_count
    bufs = {}
    sites = None
    if want_sites:
        for name in ("fst", "dxy", "pi1", "pi2", "num", "den"):
            bufs[name] = DeviceBuffer(m.device, 8 * rows)
        bufs["alt"] = DeviceBuffer(m.device, 4 * 2 * rows)
        bufs["called"] = DeviceBuffer(m.device, 4 * 2 * rows)
        sites = _abi.HudsonSites(*(bufs[n].ptr for n in ("fst", "dxy", "pi1", "pi2", "num", "den", "alt", "called")))
    totals = _abi.HudsonTotals()
    _abi.check(_abi.load().fmh_hudson_sweep(m._h, g._h, row_begin, rows, formula,
                                            C.byref(sites) if sites is not None else None, C.byref(totals), stream))
    out_sites = None
    if want_sites:
        out_sites = {n: bufs[n].to_numpy(np.float64, rows) for n in ("fst", "dxy", "pi1", "pi2", "num", "den")}
        out_sites["alt"] = bufs["alt"].to_numpy(np.uint32, 2 * rows).reshape(2, rows)
        out_sites["called"] = bufs["called"].to_numpy(np.uint32, 2 * rows).reshape(2, rows)
    return HudsonResult(hudson_totals_dict(totals), [_pop_totals(totals.pop[0]), _pop_totals(totals.pop[1])], out_sites)


def hudson_from_counts(device: int, called1: "DeviceBuffer", alt1: "DeviceBuffer", capacity1: int, called2: "DeviceBuffer", alt2: "DeviceBuffer",
                       capacity2: int, rows: int, formula: int, any_missing: bool = False, want_sites: bool = True) -> HudsonResult:
    """fmh_hudson_from_counts: the Hudson pair of two populations from their per-site count tables (u32 device arrays of `rows` entries)."""
    bufs = {}
    sites = None
    if want_sites:
        for name in ("fst", "dxy", "pi1", "pi2", "num", "den"):
            bufs[name] = DeviceBuffer(device, 8 * rows)
        bufs["alt"] = DeviceBuffer(device, 4 * 2 * rows)
        bufs["called"] = DeviceBuffer(device, 4 * 2 * rows)
        sites = _abi.HudsonSites(*(bufs[n].ptr for n in ("fst", "dxy", "pi1", "pi2", "num", "den", "alt", "called")))
    totals = _abi.HudsonTotals()
    _abi.check(_abi.load().fmh_hudson_from_counts(device, called1.ptr, alt1.ptr, capacity1, called2.ptr, alt2.ptr, capacity2, rows, formula,
                                                  1 if any_missing else 0, C.byref(sites) if sites is not None else None, C.byref(totals), None))
    out_sites = None
    if want_sites:
        out_sites = {n: bufs[n].to_numpy(np.float64, rows) for n in ("fst", "dxy", "pi1", "pi2", "num", "den")}
        out_sites["alt"] = bufs["alt"].to_numpy(np.uint32, 2 * rows).reshape(2, rows)
        out_sites["called"] = bufs["called"].to_numpy(np.uint32, 2 * rows).reshape(2, rows)
    return HudsonResult(hudson_totals_dict(totals), [_pop_totals(totals.pop[0]), _pop_totals(totals.pop[1])], out_sites)


@dataclass
class DiversityResult:
    totals: Dict[str, float]
    pi: np.ndarray
    theta: np.ndarray
    called: np.ndarray
    distinct: np.ndarray


def diversity_sites(m: DeviceMatrix, g: Groups, row_begin: int = 0, row_count: Optional[int] = None, stream=None) -> DiversityResult:
    rows = m.variants - row_begin if row_count is None else row_count
    d_pi, d_th = DeviceBuffer(m.device, 8 * rows), DeviceBuffer(m.device, 8 * rows)
    d_ca, d_di = DeviceBuffer(m.device, 4 * rows), DeviceBuffer(m.device, 4 * rows)
    totals = _abi.PopTotals()
    _abi.check(_abi.load().fmh_diversity_sites(m._h, g._h, row_begin, rows, d_pi.ptr, d_th.ptr, d_ca.ptr, d_di.ptr,
                                               C.byref(totals), stream))
    return DiversityResult(_pop_totals(totals), d_pi.to_numpy(np.float64, rows), d_th.to_numpy(np.float64, rows),
                           d_ca.to_numpy(np.uint32, rows), d_di.to_numpy(np.uint32, rows))


@dataclass
class WcResult:
    sum_a: np.ndarray  # [1+npairs]
    sum_b: np.ndarray
    informative_sites: np.ndarray
    sites_attempted: int
    a: np.ndarray  # [1+npairs][rows]
    b: np.ndarray
    state: np.ndarray
    group_called: np.ndarray  # [P][rows]


def wc_sweep(m: DeviceMatrix, g: Groups, row_begin: int = 0, row_count: Optional[int] = None, stream=None) -> WcResult:
    rows = m.variants - row_begin if row_count is None else row_count
    P = g.n_groups
    nw = 1 + P * (P - 1) // 2
    d_a, d_b = DeviceBuffer(m.device, 8 * nw * rows), DeviceBuffer(m.device, 8 * nw * rows)
    d_s, d_n = DeviceBuffer(m.device, nw * rows), DeviceBuffer(m.device, 4 * P * rows)
    totals = _abi.WcTotals()
    _abi.check(_abi.load().fmh_wc_sweep(m._h, g._h, row_begin, rows, d_a.ptr, d_b.ptr, d_s.ptr, d_n.ptr,
                                        C.byref(totals), stream))
    return WcResult(np.array(totals.sum_a[:nw]), np.array(totals.sum_b[:nw]),
                    np.array(totals.informative_sites[:nw], dtype=np.uint64), int(totals.sites_attempted),
                    d_a.to_numpy(np.float64, nw * rows).reshape(nw, rows),
                    d_b.to_numpy(np.float64, nw * rows).reshape(nw, rows),
                    d_s.to_numpy(np.uint8, nw * rows).reshape(nw, rows),
                    d_n.to_numpy(np.uint32, P * rows).reshape(P, rows))


def wc_sweep_many(m: DeviceMatrix, masks: np.ndarray, row_begin: int = 0, row_count: Optional[int] = None, sites: bool = True, stream=None) -> WcResult:
    """fmh_wc_sweep_many: W&C for any number of groups (counting in batches of 8, arithmetic from count tables).
    sites=False: no per-site track is asked for - the regional sums come straight from the count tables (a, b, state, group_called = None)."""
    rows = m.variants - row_begin if row_count is None else row_count
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    G = int(masks.shape[0])
    nw = 1 + G * (G - 1) // 2
    if not sites:
        sum_a, sum_b = np.zeros(nw, dtype=np.float64), np.zeros(nw, dtype=np.float64)
        inf = np.zeros(nw, dtype=np.uint64)
        _abi.check(_abi.load().fmh_wc_sweep_many(m._h, _ptr(masks), G, row_begin, rows, None, None, None, None, _ptr(sum_a), _ptr(sum_b), _ptr(inf), stream))
        return WcResult(sum_a, sum_b, inf, int(rows), None, None, None, None)
    d_a, d_b = DeviceBuffer(m.device, 8 * nw * rows), DeviceBuffer(m.device, 8 * nw * rows)
    d_s, d_n = DeviceBuffer(m.device, nw * rows), DeviceBuffer(m.device, 4 * G * rows)
    sum_a, sum_b = np.zeros(nw, dtype=np.float64), np.zeros(nw, dtype=np.float64)
    inf = np.zeros(nw, dtype=np.uint64)
    _abi.check(_abi.load().fmh_wc_sweep_many(m._h, _ptr(masks), G, row_begin, rows, d_a.ptr, d_b.ptr, d_s.ptr, d_n.ptr,
                                             _ptr(sum_a), _ptr(sum_b), _ptr(inf), stream))
    return WcResult(sum_a, sum_b, inf, int(rows),
                    d_a.to_numpy(np.float64, nw * rows).reshape(nw, rows),
                    d_b.to_numpy(np.float64, nw * rows).reshape(nw, rows),
                    d_s.to_numpy(np.uint8, nw * rows).reshape(nw, rows),
                    d_n.to_numpy(np.uint32, G * rows).reshape(G, rows))


def pairwise_differences(m: DeviceMatrix, n_samples: int, stream=None):
    """fmh_pairwise_differences -> (diff, both) as [n, n] uint64 arrays (upper triangle filled).  The accumulators are zeroed on the
    stream the call runs on: fmh_device_zero does not synchronise, and a stream of the caller's is not ordered behind the NULL stream."""
    n = int(n_samples)
    d_diff, d_both = DeviceBuffer(m.device, 8 * n * n), DeviceBuffer(m.device, 8 * n * n)
    lib = _abi.load()
    if n:
        _abi.check(lib.fmh_device_zero(m.device, d_diff.ptr, 8 * n * n, stream))
        _abi.check(lib.fmh_device_zero(m.device, d_both.ptr, 8 * n * n, stream))
    _abi.check(lib.fmh_pairwise_differences(m._h, n, d_diff.ptr, d_both.ptr, stream))
    return d_diff.to_numpy(np.uint64, n * n).reshape(n, n), d_both.to_numpy(np.uint64, n * n).reshape(n, n)


# ---- haplotype PCA (src/pca.rs) -----------------------------------------------------------------------------------------------
PCA_SITE_UNCALLED = 1
PCA_SITE_HIGH_ALLELE = 2


def pca_scan_sites(m: DeviceMatrix, row_begin: int = 0, row_count: Optional[int] = None, stream=None):
    """fmh_pca_scan_sites: per row the count of called allele-1 entries (uint32) and the PCA_SITE_* flags (uint8)."""
    rc = m.variants - row_begin if row_count is None else row_count
    d_alt, d_flags = DeviceBuffer(m.device, max(4 * rc, 4)), DeviceBuffer(m.device, max(rc, 1))
    _abi.check(_abi.load().fmh_pca_scan_sites(m._h, row_begin, rc, d_alt.ptr, d_flags.ptr, stream))
    return d_alt.to_numpy(np.uint32, rc), d_flags.to_numpy(np.uint8, rc)


def pca_gram_device(m: DeviceMatrix, kept_rows, set_value, clear_value, stream=None) -> DeviceBuffer:
    """fmh_pca_gram into a fresh device buffer of (samples * 2) ** 2 doubles."""
    kept = np.ascontiguousarray(kept_rows, dtype=np.uint64)
    hi = np.ascontiguousarray(set_value, dtype=np.float64)
    lo = np.ascontiguousarray(clear_value, dtype=np.float64)
    if not (kept.size == hi.size == lo.size):
        raise ValueError("kept_rows, set_value and clear_value must have one entry per kept site")
    n = m.samples * 2
    d_gram = DeviceBuffer(m.device, max(8 * n * n, 8))
    _abi.check(_abi.load().fmh_pca_gram(m._h, _ptr(kept), kept.size, _ptr(hi), _ptr(lo), d_gram.ptr, stream))
    return d_gram


def pca_gram(m: DeviceMatrix, kept_rows, set_value, clear_value, stream=None) -> np.ndarray:
    """The standardised haplotype Gram Z Z^T / (n - 1) as an (n, n) float64 array."""
    n = m.samples * 2
    return pca_gram_device(m, kept_rows, set_value, clear_value, stream).to_numpy(np.float64, n * n).reshape(n, n)


def pca_gram_sharded_device(comm, m: DeviceMatrix, kept_rows, set_value, clear_value) -> DeviceBuffer:
    """fmh_pca_gram_sharded: this rank's slab matrix `m` and the kept rows of that slab (possibly none) in, the Gram summed over the
    ranks of `comm` (a sharding.Comm) out, in a fresh device buffer.  Collective: every rank calls it."""
    kept = np.ascontiguousarray(kept_rows, dtype=np.uint64)
    hi = np.ascontiguousarray(set_value, dtype=np.float64)
    lo = np.ascontiguousarray(clear_value, dtype=np.float64)
    if not (kept.size == hi.size == lo.size):
        raise ValueError("kept_rows, set_value and clear_value must have one entry per kept site")
    n = m.samples * 2
    d_gram = DeviceBuffer(m.device, max(8 * n * n, 8))
    _abi.check(_abi.load().fmh_pca_gram_sharded(comm._h, m._h, _ptr(kept), kept.size, _ptr(hi), _ptr(lo), d_gram.ptr, None))
    return d_gram


def pca_gram_sharded(comm, m: DeviceMatrix, kept_rows, set_value, clear_value) -> np.ndarray:
    """The same as an (n, n) float64 array."""
    n = m.samples * 2
    return pca_gram_sharded_device(comm, m, kept_rows, set_value, clear_value).to_numpy(np.float64, n * n).reshape(n, n)


def pca_eigen_scores(device: int, gram, n_components: int):
    """fmh_pca_eigen_scores of a symmetric (n, n) array or of a DeviceBuffer holding one (overwritten): (eigenvalues descending
    [n_components], scores [n][n_components])."""
    if isinstance(gram, DeviceBuffer):
        buf, n = gram, int(round((gram.nbytes // 8) ** 0.5))
    else:
        a = np.ascontiguousarray(gram, dtype=np.float64)
        buf, n = DeviceBuffer.from_numpy(device, a), a.shape[0]
    values, scores = np.empty(n_components, dtype=np.float64), np.empty((n, n_components), dtype=np.float64)
    _abi.check(_abi.load().fmh_pca_eigen_scores(device, buf.ptr, n, n_components, _ptr(values), _ptr(scores)))
    return values, scores


# ---- linkage disequilibrium ------------------------------------------------------------------------------------------------------
@dataclass
class LdBandResult:
    r2: Optional[np.ndarray]       # [rows][band] float64
    n_ab: Optional[np.ndarray]     # [rows][band] uint32
    n_joint: Optional[np.ndarray]
    over: Optional[np.ndarray]     # [rows][ceil(band / 32)] uint32
    site_n: Optional[np.ndarray]   # [rows] uint32
    site_alt: Optional[np.ndarray]


def ld_band(m: DeviceMatrix, g: Optional[Groups], band: int, threshold: float = 0.0, row_begin: int = 0, row_count: Optional[int] = None,
            partner_end: Optional[int] = None, want=("r2", "n_ab", "n_joint", "over", "site_n", "site_alt"), stream=None) -> LdBandResult:
    """fmh_ld_band: r^2 and its counts between rows [row_begin, row_begin + row_count) and their next `band` rows below partner_end
    (default: the end of the rows asked for); `want` names the outputs to ask for."""
    rows = m.variants - row_begin if row_count is None else row_count
    pend = row_begin + rows if partner_end is None else partner_end
    band, words = int(band), (int(band) + 31) // 32
    sizes = {"r2": 8 * rows * band, "n_ab": 4 * rows * band, "n_joint": 4 * rows * band, "over": 4 * rows * words, "site_n": 4 * rows, "site_alt": 4 * rows}
    bufs = {k: DeviceBuffer(m.device, max(sizes[k], 4)) for k in want}
    out = _abi.LdBandOut(*(bufs[k].ptr if k in bufs else None for k in ("r2", "n_ab", "n_joint", "over")))
    _abi.check(_abi.load().fmh_ld_band(m._h, g._h if g is not None else None, row_begin, rows, pend, band, float(threshold), C.byref(out),
                                       bufs["site_n"].ptr if "site_n" in bufs else None, bufs["site_alt"].ptr if "site_alt" in bufs else None, stream))

    def fetch(k, dtype, shape):
        return bufs[k].to_numpy(dtype, int(np.prod(shape))).reshape(shape) if k in bufs else None

    return LdBandResult(fetch("r2", np.float64, (rows, band)), fetch("n_ab", np.uint32, (rows, band)), fetch("n_joint", np.uint32, (rows, band)),
                        fetch("over", np.uint32, (rows, words)), fetch("site_n", np.uint32, (rows,)), fetch("site_alt", np.uint32, (rows,)))


def ld_prune(m: DeviceMatrix, g: Optional[Groups], window: int, threshold: float, row_begin: int = 0, row_count: Optional[int] = None,
             chunk_rows: int = 0, stream=None) -> np.ndarray:
    """fmh_ld_prune (fmh_ld_prune_chunked when chunk_rows is given): the forward greedy keep flags of the rows, as bool."""
    rows = m.variants - row_begin if row_count is None else row_count
    keep = np.zeros(rows, dtype=np.uint8)
    _abi.check(_abi.load().fmh_ld_prune_chunked(m._h, g._h if g is not None else None, row_begin, rows, int(window), float(threshold), _ptr(keep),
                                                int(chunk_rows), stream))
    return keep.astype(bool)


def ld_prune_bits(over: np.ndarray, band: int) -> np.ndarray:
    """fmh_ld_prune_bits: the greedy rule over an `over` band [rows][ceil(band / 32)] on the host (no device)."""
    over = np.ascontiguousarray(over, dtype=np.uint32)
    rows = over.shape[0]
    keep = np.zeros(rows, dtype=np.uint8)
    _abi.check(_abi.load().fmh_ld_prune_bits(_ptr(over), rows, int(band), _ptr(keep)))
    return keep.astype(bool)


# ---- site frequency spectra --------------------------------------------------------------------------------------------------------
SFS_DEFAULT_ITEM_ROWS = 4096         # FMH_SFS_ITEM_ROWS unset
SFS_DEFAULT_LDS_BINS = 5120 - 4      # FMH_SFS_LDS_BINS unset: an eighth of a CU's 160 KiB in u32 bins less the kernel's 16-byte head
SFS_MAX_LDS_BINS = 40960 - 4         # the largest cap the option takes: the whole 160 KiB, one 512-thread workgroup per CU


@dataclass
class SfsResult:
    counts: np.ndarray         # [n_windows][n + 1] uint64
    multiallelic: np.ndarray   # [n_windows] uint64
    incomplete: np.ndarray


@dataclass
class SfsJointResult:
    counts: np.ndarray         # [n0 + 1][n1 + 1] uint64
    multiallelic: int
    incomplete: int


def _skipped_arrays(skipped, count: int):
    flat = np.ctypeslib.as_array(skipped).view(np.uint64).reshape(count, 2) if count else np.zeros((0, 2), dtype=np.uint64)
    return flat[:, 0].copy(), flat[:, 1].copy()


def sfs(m: DeviceMatrix, g: Groups, windows=None, stream=None) -> SfsResult:
    """fmh_sfs: the 1-D spectra of the one group of `g` over row windows [(begin, end), ...] (default: one window, every row)."""
    w = np.array([[0, m.variants]] if windows is None else windows, dtype=np.uint64).reshape(-1, 2)
    n_windows, width = w.shape[0], g.sizes[0] + 1
    skipped = (_abi.SfsSkipped * max(n_windows, 1))()
    d_sfs = DeviceBuffer(m.device, max(8 * n_windows * width, 8))
    _abi.check(_abi.load().fmh_sfs(m._h, g._h, _ptr(w), n_windows, d_sfs.ptr, skipped, stream))
    multi, incomplete = _skipped_arrays(skipped, n_windows)
    return SfsResult(d_sfs.to_numpy(np.uint64, n_windows * width).reshape(n_windows, width), multi, incomplete)


def sfs_joint(m: DeviceMatrix, g: Groups, row_begin: int = 0, row_count: Optional[int] = None, stream=None) -> SfsJointResult:
    """fmh_sfs_joint: the joint spectrum [n0 + 1][n1 + 1] of the two groups of `g` over rows [row_begin, row_begin + row_count)."""
    rows = m.variants - row_begin if row_count is None else row_count
    shape = (g.sizes[0] + 1, g.sizes[1] + 1) if g.n_groups == 2 else (1, 1)
    skipped = (_abi.SfsSkipped * 1)()
    d_sfs = DeviceBuffer(m.device, 8 * shape[0] * shape[1])
    _abi.check(_abi.load().fmh_sfs_joint(m._h, g._h, row_begin, rows, d_sfs.ptr, skipped, stream))
    return SfsJointResult(d_sfs.to_numpy(np.uint64, shape[0] * shape[1]).reshape(shape), int(skipped[0].multiallelic), int(skipped[0].incomplete))


def sfs_stats(counts) -> Dict[str, float]:
    """fmh_sfs_stats (host only): the statistics of one 1-D spectrum of n + 1 bins."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    if counts.size < 1:
        raise ValueError("a spectrum has at least one bin")
    out = _abi.SfsStatsOut()
    _abi.check(_abi.load().fmh_sfs_stats(_ptr(counts), counts.size - 1, C.byref(out)))
    return {name: getattr(out, name) for name, _ in _abi.SfsStatsOut._fields_}


# ---- Patterson f-statistics ----------------------------------------------------------------------------------------------------------
FSTAT_DEFAULT_ITEM_ROWS = 4096       # FMH_FSTAT_ITEM_ROWS unset
FSTAT_DEFAULT_LDS_MASK_BYTES = 8192  # FMH_FSTAT_LDS_MASK_BYTES unset


@dataclass
class FstatMoments:
    moments: np.ndarray        # [n_blocks][M] uint64
    multiallelic: np.ndarray   # [n_blocks] uint64
    incomplete: np.ndarray
    sizes: np.ndarray          # [G] uint64


def fstat_moment_count(n_groups: int) -> int:
    """fmh_fstat_moment_count: M = 1 + G + G (G + 1) / 2, 0 when G is outside 2..32 (needs no device)."""
    return int(_abi.load().fmh_fstat_moment_count(int(n_groups)))


def fstat_moments(m: DeviceMatrix, masks: np.ndarray, blocks=None, stream=None) -> FstatMoments:
    """fmh_fstat_moments: the moment slices of the G groups `masks` [G][columns] over row blocks [(begin, end), ...] (default: one block,
    every row)."""
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    b = np.array([[0, m.variants]] if blocks is None else blocks, dtype=np.uint64).reshape(-1, 2)
    n_blocks, width = b.shape[0], fstat_moment_count(masks.shape[0])
    skipped = (_abi.SfsSkipped * max(n_blocks, 1))()
    d_moments = DeviceBuffer(m.device, max(8 * n_blocks * width, 8))
    _abi.check(_abi.load().fmh_fstat_moments(m._h, _ptr(masks), masks.shape[0], _ptr(b), n_blocks, d_moments.ptr, skipped, stream))
    multi, incomplete = _skipped_arrays(skipped, n_blocks)
    return FstatMoments(d_moments.to_numpy(np.uint64, n_blocks * width).reshape(n_blocks, width), multi, incomplete,
                        masks.astype(bool).sum(axis=1).astype(np.uint64))


def fstat_f4(moments, sizes, a: int, b: int, c: int, d: int, unbiased: bool = True) -> float:
    """fmh_fstat_f4 (host only): the block's sum of the estimator of (p_a - p_b)(p_c - p_d) from one slice."""
    moments = np.ascontiguousarray(moments, dtype=np.uint64).reshape(-1)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
    if moments.size != fstat_moment_count(sizes.size):
        raise ValueError("one block's slice has 1 + G + G (G + 1) / 2 entries for the G sample sizes")
    out = C.c_double()
    _abi.check(_abi.load().fmh_fstat_f4(_ptr(moments), _ptr(sizes), sizes.size, a, b, c, d, int(bool(unbiased)), C.byref(out)))
    return out.value


def block_jackknife(num, den, weight=None) -> Dict[str, float]:
    """fmh_block_jackknife (host only): the weighted delete-one-block jackknife of sum(num) / sum(den)."""
    num = np.ascontiguousarray(num, dtype=np.float64).reshape(-1)
    den = np.ascontiguousarray(den, dtype=np.float64).reshape(-1)
    if weight is not None:
        weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
    if den.size != num.size or (weight is not None and weight.size != num.size):
        raise ValueError("num, den and weight have one entry per block")
    out = _abi.JackknifeOut()
    _abi.check(_abi.load().fmh_block_jackknife(_ptr(num), _ptr(den), _ptr(weight), num.size, C.byref(out)))
    return {name: getattr(out, name) for name, _ in _abi.JackknifeOut._fields_}


# ---- relatedness: KING-robust kinship ------------------------------------------------------------------------------------------------
KINSHIP_TABLES = ("both", "het_het", "ibs0", "het_hom")


@dataclass
class KinshipCounts:
    both: np.ndarray      # [n][n] uint64 each
    het_het: np.ndarray
    ibs0: np.ndarray
    het_hom: np.ndarray   # [i][j]: i het, j hom
    kept_rows: int


class KinshipBuffers:
    """The four [n][n] u64 device tables fmh_kinship_counts ADDS into, zero (or `fill`) on creation."""

    def __init__(self, device: int, n: int, fill: Optional[np.ndarray] = None):
        self.device, self.n = device, int(n)
        fill = np.zeros(self.n * self.n, dtype=np.uint64) if fill is None else np.ascontiguousarray(fill, dtype=np.uint64)
        self.bufs = [DeviceBuffer.from_numpy(device, fill) for _ in KINSHIP_TABLES]  # (a blocking copy: safe before a call on any stream)
        self.out = _abi.KinshipOut(*[b.ptr for b in self.bufs])

    def tables(self):
        return [b.to_numpy(np.uint64, self.n * self.n).reshape(self.n, self.n) for b in self.bufs]


def kinship_counts(m: DeviceMatrix, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
                   into: Optional[KinshipBuffers] = None, stream=None) -> KinshipCounts:
    """fmh_kinship_counts: the four genotype-class tables of the samples `samples` (ascending sample numbers; None = the first n_samples,
    default all) over the rows of [row_begin, row_begin + row_count) that `keep` keeps (None = all).  `into`: accumulate into these buffers."""
    rows = m.variants - row_begin if row_count is None else row_count
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.size != rows:
            raise ValueError("keep has one entry per row of the range")
    bufs = into if into is not None else KinshipBuffers(m.device, n)
    kept = C.c_uint64(0)
    _abi.check(_abi.load().fmh_kinship_counts(m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), C.byref(bufs.out), C.byref(kept), stream))
    both, het_het, ibs0, het_hom = bufs.tables()
    return KinshipCounts(both, het_het, ibs0, het_hom, int(kept.value))


def kinship_stats(both, het_het, ibs0, het_hom, ibs_distance: bool = True):
    """fmh_kinship_stats (host only): (kinship, ibs_distance or None) as [n][n] float64 from the four tables."""
    tables = [np.ascontiguousarray(t, dtype=np.uint64) for t in (both, het_het, ibs0, het_hom)]
    n = tables[0].shape[0]
    if any(t.shape != (n, n) for t in tables):
        raise ValueError("the four tables are [n][n]")
    phi = np.empty((n, n), dtype=np.float64)
    dist = np.empty((n, n), dtype=np.float64) if ibs_distance else None
    _abi.check(_abi.load().fmh_kinship_stats(*[_ptr(t) for t in tables], n, _ptr(phi), _ptr(dist)))
    return phi, dist


def kinship_unrelated(kinship, threshold: float) -> np.ndarray:
    """fmh_kinship_unrelated (host only): the greedy unrelated subset's keep flags, as bool."""
    phi = np.ascontiguousarray(kinship, dtype=np.float64)
    n = phi.shape[0]
    if phi.shape != (n, n):
        raise ValueError("kinship is [n][n]")
    keep = np.zeros(n, dtype=np.uint8)
    _abi.check(_abi.load().fmh_kinship_unrelated(_ptr(phi), n, float(threshold), _ptr(keep)))
    return keep.astype(bool)


# ---- genomic relationship matrix and its eigenpairs ---------------------------------------------------------------------------------------
GRM_METHODS = ("standardized", "centered")   # FMH_GRM_STANDARDIZED, FMH_GRM_CENTERED
GRM_DENOMINATORS = ("sites", "pairs")        # FMH_GRM_SITES, FMH_GRM_PAIRS


def grm_params(method: str = "standardized", denominator: str = "sites") -> "_abi.GrmParams":
    return _abi.GrmParams(GRM_METHODS.index(method), GRM_DENOMINATORS.index(denominator))


@dataclass
class GrmResult:
    products: np.ndarray               # S [n][n] float64
    pair_sites: Optional[np.ndarray]   # N [n][n] uint64, or None
    called: np.ndarray                 # c, a and the usable flag of the kept rows
    allele_count: np.ndarray
    usable: np.ndarray
    n_usable: int
    scale: float
    kept_rows: int


class GrmBuffers:
    """The [n][n] device matrices fmh_grm ADDS into: S (f64) and, with pairs=True, N (u64); zero (or `fill` / `fill_pairs`) on creation."""

    def __init__(self, device: int, n: int, pairs: bool = False, fill: Optional[np.ndarray] = None, fill_pairs: Optional[np.ndarray] = None):
        self.device, self.n = device, int(n)
        fill = np.zeros(self.n * self.n, dtype=np.float64) if fill is None else np.ascontiguousarray(fill, dtype=np.float64)
        self.products = DeviceBuffer.from_numpy(device, fill)
        self.pair_sites = None
        if pairs:
            fill_pairs = np.zeros(self.n * self.n, dtype=np.uint64) if fill_pairs is None else np.ascontiguousarray(fill_pairs, dtype=np.uint64)
            self.pair_sites = DeviceBuffer.from_numpy(device, fill_pairs)


def grm(m: DeviceMatrix, params=None, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
        pairs: bool = False, into: Optional[GrmBuffers] = None, stream=None) -> GrmResult:
    """fmh_grm: the products S (and with `pairs` the pair counts N) of the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all) over the usable rows among those of [row_begin, row_begin + row_count) that `keep` keeps.  `into`: accumulate."""
    params = grm_params() if params is None else params
    rows = m.variants - row_begin if row_count is None else row_count
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.size != rows:
            raise ValueError("keep has one entry per row of the range")
    bufs = into if into is not None else GrmBuffers(m.device, n, pairs or params.denominator == 1)
    called, allele_count, usable = np.zeros(max(rows, 1), np.uint32), np.zeros(max(rows, 1), np.uint32), np.zeros(max(rows, 1), np.uint8)
    n_usable, scale, kept = C.c_uint64(0), C.c_double(0.0), C.c_uint64(0)
    out = _abi.GrmOut(bufs.products.ptr, None if bufs.pair_sites is None else bufs.pair_sites.ptr, _ptr(called), _ptr(allele_count), _ptr(usable),
                      C.pointer(n_usable), C.pointer(scale))
    _abi.check(_abi.load().fmh_grm(m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), C.byref(params), C.byref(out), C.byref(kept), stream))
    k = int(kept.value)
    S = bufs.products.to_numpy(np.float64, n * n).reshape(n, n)
    N = None if bufs.pair_sites is None else bufs.pair_sites.to_numpy(np.uint64, n * n).reshape(n, n)
    return GrmResult(S, N, called[:k], allele_count[:k], usable[:k].astype(bool), int(n_usable.value), float(scale.value), k)


def grm_values(called, allele_count, method: str = "standardized"):
    """fmh_grm_values (host only): (usable bool [rows], p [rows], z [rows][3], scale, n_usable) from the exact counts."""
    c, a = np.ascontiguousarray(called, dtype=np.uint32), np.ascontiguousarray(allele_count, dtype=np.uint32)
    if c.shape != a.shape or c.ndim != 1:
        raise ValueError("called and allele_count are one-dimensional and of one length")
    rows = c.size
    usable, p, z = np.zeros(rows, np.uint8), np.zeros(rows, np.float64), np.zeros((rows, 3), np.float64)
    scale, n_usable = C.c_double(0.0), C.c_uint64(0)
    _abi.check(_abi.load().fmh_grm_values(_ptr(c), _ptr(a), rows, GRM_METHODS.index(method), _ptr(usable), _ptr(p), _ptr(z), C.byref(scale), C.byref(n_usable)))
    return usable.astype(bool), p, z, float(scale.value), int(n_usable.value)


def grm_finish(products, pair_sites, n_usable: int, scale: float, params=None) -> np.ndarray:
    """fmh_grm_finish (host only): A [n][n] from S (and N for denominator "pairs")."""
    params = grm_params() if params is None else params
    S = np.ascontiguousarray(products, dtype=np.float64)
    n = S.shape[0]
    N = None if pair_sites is None else np.ascontiguousarray(pair_sites, dtype=np.uint64)
    if S.shape != (n, n) or (N is not None and N.shape != (n, n)):
        raise ValueError("products and pair_sites are [n][n]")
    A = np.empty((n, n), dtype=np.float64)
    _abi.check(_abi.load().fmh_grm_finish(_ptr(S), _ptr(N), n, C.byref(params), int(n_usable), float(scale), _ptr(A)))
    return A


def grm_host(dosage, method: str = "standardized"):
    """fmh_grm_host (host only): (S, N, n_usable, scale) from a [K][n] dosage table (0, 1, 2; above 2 = not called)."""
    d = np.ascontiguousarray(dosage, dtype=np.uint8)
    K, n = d.shape
    S, N = np.empty((n, n), dtype=np.float64), np.empty((n, n), dtype=np.uint64)
    n_usable, scale = C.c_uint64(0), C.c_double(0.0)
    _abi.check(_abi.load().fmh_grm_host(_ptr(d), K, n, GRM_METHODS.index(method), _ptr(S), _ptr(N), C.byref(n_usable), C.byref(scale)))
    return S, N, int(n_usable.value), float(scale.value)


def grm_eigen(device: int, matrix, n_components: int):
    """fmh_grm_eigen of a symmetric (n, n) array: (eigenvalues descending [n_components], unit eigenvectors [n][n_components], the component
    of the largest magnitude positive)."""
    a = np.ascontiguousarray(matrix, dtype=np.float64)
    n = a.shape[0]
    buf = DeviceBuffer.from_numpy(device, a)
    values, vectors = np.empty(n_components, dtype=np.float64), np.empty((n, n_components), dtype=np.float64)
    _abi.check(_abi.load().fmh_grm_eigen(device, buf.ptr, n, n_components, _ptr(values), _ptr(vectors)))
    return values, vectors


# ---- mixed-model association scan ----------------------------------------------------------------------------------------------------------
LMM_DEFAULT_ITEM_ROWS = 4096   # FMH_LMM_ITEM_ROWS unset: at most
LMM_GRID_POINTS = 101


@dataclass
class LmmProjections:
    quad: np.ndarray           # [rows][P] float64
    lin: np.ndarray            # [rows][L] float64
    called: np.ndarray         # c, a per row, uint32
    allele_count: np.ndarray


def lmm_projections(m: DeviceMatrix, basis, weights, linear, samples=None, n_samples: Optional[int] = None, row_begin: int = 0,
                    row_count: Optional[int] = None, stream=None, fill: Optional[float] = None) -> LmmProjections:
    """fmh_lmm_projections over rows [row_begin, row_begin + row_count) for the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all).  basis [n][K], weights [P][K], linear [L][K] float64.  `fill` pre-fills the outputs (tests: every entry is written)."""
    rows = m.variants - row_begin if row_count is None else row_count
    basis, weights, linear = (np.ascontiguousarray(a, dtype=np.float64) for a in (basis, weights, linear))
    if basis.ndim != 2 or weights.ndim != 2 or linear.ndim != 2 or weights.shape[1] != basis.shape[1] or linear.shape[1] != basis.shape[1]:
        raise ValueError("basis is [n][K], weights [P][K], linear [L][K]")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if basis.shape[0] != n:
        raise ValueError("basis has one row per selected sample")
    K, P, L = basis.shape[1], weights.shape[0], linear.shape[0]
    bufs = [DeviceBuffer.from_numpy(m.device, a) for a in (basis, weights, linear)]
    start = np.zeros(max(rows, 1) * (P + L), dtype=np.float64) if fill is None else np.full(max(rows, 1) * (P + L), fill, dtype=np.float64)
    d_quad = DeviceBuffer.from_numpy(m.device, start[: max(rows, 1) * P])
    d_lin = DeviceBuffer.from_numpy(m.device, start[: max(rows, 1) * L])
    called, allele_count = np.zeros(max(rows, 1), np.uint32), np.zeros(max(rows, 1), np.uint32)
    _abi.check(_abi.load().fmh_lmm_projections(m._h, _ptr(samples), n, row_begin, rows, bufs[0].ptr, K, bufs[1].ptr, P, bufs[2].ptr, L, d_quad.ptr, d_lin.ptr,
                                               _ptr(called), _ptr(allele_count), stream))
    return LmmProjections(d_quad.to_numpy(np.float64, rows * P).reshape(rows, P), d_lin.to_numpy(np.float64, rows * L).reshape(rows, L), called[:rows],
                          allele_count[:rows])


def lmm_projections_host(dosage, basis, weights, linear) -> LmmProjections:
    """fmh_lmm_projections_host (host only): the twin over a [rows][n] dosage table (0, 1, 2; above 2 = not called)."""
    d = np.ascontiguousarray(dosage, dtype=np.uint8)
    basis, weights, linear = (np.ascontiguousarray(a, dtype=np.float64) for a in (basis, weights, linear))
    rows, n = d.shape
    K, P, L = basis.shape[1], weights.shape[0], linear.shape[0]
    quad, lin = np.empty((rows, P), dtype=np.float64), np.empty((rows, L), dtype=np.float64)
    called, allele_count = np.zeros(rows, np.uint32), np.zeros(rows, np.uint32)
    _abi.check(_abi.load().fmh_lmm_projections_host(_ptr(d), rows, n, _ptr(basis), K, _ptr(weights), P, _ptr(linear), L, _ptr(quad), _ptr(lin), _ptr(called),
                                                    _ptr(allele_count)))
    return LmmProjections(quad, lin, called, allele_count)


# ---- admixture -------------------------------------------------------------------------------------------------------------------------------
ADMIX_MAX_K = 16
ADMIX_EPS = 1e-5
ADMIX_PASS_ROWS = 128   # FMH_ADMIX_ITEM_ROWS is rounded up to whole passes
ADMIX_UPDATE_Q, ADMIX_UPDATE_F = 1, 2


def _admix_flags(update_q: bool, update_f: bool) -> int:
    return (ADMIX_UPDATE_Q if update_q else 0) | (ADMIX_UPDATE_F if update_f else 0)


class AdmixImage:
    """fmh_admix: the resident 2-bit genotype image of the usable rows among those of [row_begin, row_begin + row_count) that `keep` keeps, for
    the samples `samples` (ascending sample numbers; None = the first n_samples, default all).  Holds n, kept_rows, m and the host tracks
    usable (bool), called, allele_count per kept row and sample_sites [n].  A context manager; close() frees the device memory."""

    def __init__(self, m: DeviceMatrix, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
                 stream=None):
        rows = m.variants - row_begin if row_count is None else row_count
        if samples is not None:
            samples = np.ascontiguousarray(samples, dtype=np.uint32)
            n = samples.size
        else:
            n = m.samples if n_samples is None else int(n_samples)
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if keep.size != rows:
                raise ValueError("keep has one entry per row of the range")
        self._h = None
        self.device = m.device
        h = C.c_void_p()
        _abi.check(_abi.load().fmh_admix_create(m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), C.byref(h), stream))
        self._h = h.value
        info = _abi.AdmixInfoOut()
        _abi.check(_abi.load().fmh_admix_info(self._h, C.byref(info)))
        self.n, self.kept_rows, self.m = int(info.n_samples), int(info.kept_rows), int(info.usable_rows)

        def copy(ptr, dtype, count):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,)).copy()

        self.usable = copy(info.h_usable, np.uint8, self.kept_rows).astype(bool)
        self.called = copy(info.h_called, np.uint32, self.kept_rows)
        self.allele_count = copy(info.h_allele_count, np.uint32, self.kept_rows)
        self.sample_sites = copy(info.h_sample_sites, np.uint64, self.n)

    def close(self):
        if getattr(self, "_h", None):
            _abi.load().fmh_admix_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _admix_state(q, f):
    q, f = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(f, dtype=np.float64)
    if q.ndim != 2 or f.ndim != 2 or q.shape[1] != f.shape[1]:
        raise ValueError("q is [n][K] and f is [m][K]")
    return q, f


def admix_step(image: AdmixImage, q, f, loglik: bool = True, update_q: bool = True, update_f: bool = True, stream=None, fill: Optional[float] = None):
    """fmh_admix_step: one EM step from q [n][K], f [m][K]: (q', f', l of the input or None).  `fill` pre-fills the outputs (tests: every entry is
    written)."""
    q, f = _admix_state(q, f)
    if q.shape[0] != image.n or f.shape[0] != image.m:
        raise ValueError("q has one row per sample of the image and f one per usable row")
    K = q.shape[1]
    d_q, d_f = DeviceBuffer.from_numpy(image.device, q), DeviceBuffer.from_numpy(image.device, f)
    d_qo = DeviceBuffer.from_numpy(image.device, np.full(q.size, 0.0 if fill is None else fill, dtype=np.float64))
    d_fo = DeviceBuffer.from_numpy(image.device, np.full(f.size, 0.0 if fill is None else fill, dtype=np.float64))
    ll = C.c_double(0.0)
    _abi.check(_abi.load().fmh_admix_step(image._h, K, d_q.ptr, d_f.ptr, d_qo.ptr, d_fo.ptr, C.byref(ll) if loglik else None, _admix_flags(update_q, update_f),
                                         stream))
    return d_qo.to_numpy(np.float64, q.size).reshape(q.shape), d_fo.to_numpy(np.float64, f.size).reshape(f.shape), float(ll.value) if loglik else None


@dataclass
class AdmixTracks:
    usable: np.ndarray         # bool [rows]
    called: np.ndarray         # c, a per row, uint32
    allele_count: np.ndarray
    sample_sites: np.ndarray   # m_i, uint64 [n]
    m: int


def admix_tracks_host(dosage) -> AdmixTracks:
    """fmh_admix_step_host without a state (host only): the tracks of a [rows][n] dosage table (0, 1, 2; above 2 = not called)."""
    d = np.ascontiguousarray(dosage, dtype=np.uint8)
    rows, n = d.shape
    usable, called, allele_count, sites = np.zeros(rows, np.uint8), np.zeros(rows, np.uint32), np.zeros(rows, np.uint32), np.zeros(n, np.uint64)
    m = C.c_uint64(0)
    tracks = _abi.AdmixTracks(_ptr(usable), _ptr(called), _ptr(allele_count), _ptr(sites), C.pointer(m))
    _abi.check(_abi.load().fmh_admix_step_host(_ptr(d), rows, n, 0, None, None, None, None, None, 0, C.byref(tracks)))
    return AdmixTracks(usable.astype(bool), called, allele_count, sites, int(m.value))


def admix_step_host(dosage, q, f, loglik: bool = True, update_q: bool = True, update_f: bool = True):
    """fmh_admix_step_host (host only): the twin over a [rows][n] dosage table; f is [m][K] over the usable rows: (q', f', l or None)."""
    d = np.ascontiguousarray(dosage, dtype=np.uint8)
    q, f = _admix_state(q, f)
    rows, n = d.shape
    if q.shape[0] != n or f.shape[0] != admix_tracks_host(d).m:
        raise ValueError("q has one row per sample and f one per usable row")
    K = q.shape[1]
    q_out, f_out = np.full(q.shape, np.nan), np.full(f.shape, np.nan)
    ll = C.c_double(0.0)
    _abi.check(_abi.load().fmh_admix_step_host(_ptr(d), rows, n, K, _ptr(q), _ptr(f), _ptr(q_out), _ptr(f_out), C.byref(ll) if loglik else None,
                                              _admix_flags(update_q, update_f), None))
    return q_out, f_out, float(ll.value) if loglik else None


def admix_start(called, allele_count, n: int, k: int, seed: int = 0):
    """fmh_admix_start (host only): the default start (q [n][k], f [m][k]) from c, a of the m usable rows."""
    c, a = np.ascontiguousarray(called, dtype=np.uint32), np.ascontiguousarray(allele_count, dtype=np.uint32)
    if c.shape != a.shape or c.ndim != 1:
        raise ValueError("called and allele_count are one-dimensional and of one length")
    q, f = np.empty((int(n), int(k)), dtype=np.float64), np.empty((c.size, int(k)), dtype=np.float64)
    _abi.check(_abi.load().fmh_admix_start(_ptr(c), _ptr(a), c.size, int(n), int(k), int(seed), _ptr(q), _ptr(f)))
    return q, f


def admix_accelerate(state0, state1, state2):
    """fmh_admix_accelerate (host only): states are (q, f) pairs; returns (qa, fa, alpha); alpha = 0: nothing to extrapolate, the state is state2's."""
    (q0, f0), (q1, f1), (q2, f2) = (_admix_state(*s) for s in (state0, state1, state2))
    if not (q0.shape == q1.shape == q2.shape and f0.shape == f1.shape == f2.shape):
        raise ValueError("the three states have one shape")
    qa, fa = np.empty_like(q0), np.empty_like(f0)
    alpha = C.c_double(0.0)
    _abi.check(_abi.load().fmh_admix_accelerate(_ptr(q0), _ptr(f0), _ptr(q1), _ptr(f1), _ptr(q2), _ptr(f2), q0.shape[0], f0.shape[0], q0.shape[1], _ptr(qa),
                                               _ptr(fa), C.byref(alpha)))
    return qa, fa, float(alpha.value)


@dataclass
class LmmNull:
    q: int
    dropped: np.ndarray        # [c_in] bool
    delta: np.ndarray          # [P]
    sigma_g2: np.ndarray
    sigma_e2: np.ndarray
    heritability: np.ndarray
    log_likelihood: np.ndarray
    at_boundary: np.ndarray    # [P] bool
    reason: np.ndarray         # [P] uint8
    weights: np.ndarray        # [P][n]
    linear: np.ndarray         # [P * (q + 1)][n]
    M: np.ndarray              # [P][q][q]
    v: np.ndarray              # [P][q]
    R: np.ndarray              # [P]
    grid_log_likelihood: np.ndarray  # [P][101]


def lmm_null(eigenvalues, eigenvectors, phenotypes, covariates=None, fixed_delta=None) -> LmmNull:
    """fmh_lmm_null (host only): the null fit per phenotype; `fixed_delta` [P] skips the search."""
    lam = np.ascontiguousarray(eigenvalues, dtype=np.float64)
    U = np.ascontiguousarray(eigenvectors, dtype=np.float64)
    y = np.ascontiguousarray(phenotypes, dtype=np.float64)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    n, P = y.shape
    if lam.shape != (n,) or U.shape != (n, n):
        raise ValueError("eigenvalues are [n], eigenvectors [n][n], phenotypes [n][P]")
    cov = None if covariates is None else np.ascontiguousarray(covariates, dtype=np.float64).reshape(n, -1)
    cin = 0 if cov is None else cov.shape[1]
    fixed = None if fixed_delta is None else np.ascontiguousarray(fixed_delta, dtype=np.float64).reshape(P)
    qmax = cin + 1
    f = lambda *shape: np.zeros(shape, dtype=np.float64)
    delta, sg, se, h2, ll, R = f(P), f(P), f(P), f(P), f(P), f(P)
    boundary, reason, dropped = np.zeros(P, np.uint8), np.zeros(P, np.uint8), np.zeros(max(cin, 1), np.uint8)
    weights, linear, M, v, grid = f(P * n), f(P * (qmax + 1) * n), f(P * qmax * qmax), f(P * qmax), f(P, LMM_GRID_POINTS)
    out = _abi.LmmNullOut(*(a.ctypes.data for a in (delta, sg, se, h2, ll, boundary, reason, weights, linear, M, v, R, grid)))
    q = C.c_size_t(0)
    _abi.check(_abi.load().fmh_lmm_null(_ptr(lam), _ptr(U), _ptr(y), _ptr(cov), n, P, cin, _ptr(fixed), C.byref(q), _ptr(dropped), C.byref(out)))
    q = int(q.value)
    return LmmNull(q, dropped[:cin].astype(bool), delta, sg, se, h2, ll, boundary.astype(bool), reason, weights.reshape(P, n),
                   linear[: P * (q + 1) * n].reshape(P * (q + 1), n), M[: P * q * q].reshape(P, q, q), v[: P * q].reshape(P, q), R, grid)


def lmm_stats(quad, lin, called, allele_count, M, v, R, n_samples: int):
    """fmh_lmm_stats (host only): dict(beta, se, t, p) [rows][P] from the projections and the null fit's M [P][q][q], v [P][q], R [P]."""
    quad, lin = np.ascontiguousarray(quad, dtype=np.float64), np.ascontiguousarray(lin, dtype=np.float64)
    M, v, R = (np.ascontiguousarray(a, dtype=np.float64) for a in (M, v, R))
    c, a = np.ascontiguousarray(called, dtype=np.uint32), np.ascontiguousarray(allele_count, dtype=np.uint32)
    rows, P = quad.shape
    q = v.shape[1]
    if lin.shape != (rows, P * (q + 1)) or M.shape != (P, q, q) or R.shape != (P,) or c.shape != (rows,) or a.shape != (rows,):
        raise ValueError("quad is [rows][P], lin [rows][P (q + 1)], M [P][q][q], v [P][q], R [P]")
    out = {k: np.empty((rows, P), dtype=np.float64) for k in ("beta", "se", "t", "p")}
    _abi.check(_abi.load().fmh_lmm_stats(_ptr(quad), _ptr(lin), _ptr(c), _ptr(a), rows, _ptr(M), _ptr(v), _ptr(R), int(n_samples), q, P, _ptr(out["beta"]),
                                         _ptr(out["se"]), _ptr(out["t"]), _ptr(out["p"])))
    return out


# ---- genotype QC: class counts per site and per sample, HWE exact test -----------------------------------------------------------------
QC_DEFAULT_ITEM_ROWS = 4096   # FMH_QC_ITEM_ROWS unset
QC_CLASSES = ("hom_ref", "het", "hom_alt")
QC_SITE_STATS = ("call_rate", "alt_frequency", "maf", "f_is", "expected_het")
QC_SAMPLE_STATS = ("call_rate", "het_rate", "f")


@dataclass
class GenotypeCounts:
    site: Optional[Dict[str, np.ndarray]]      # hom_ref, het, hom_alt: [row_count] uint32 (a track not asked for is absent), or None
    sample: Optional[Dict[str, np.ndarray]]    # hom_ref, het, hom_alt and / or weighted_called: [n] uint64, or None
    kept_rows: int


class GenotypeSampleBuffers:
    """The [n] u64 device tables fmh_genotype_counts ADDS into, zero (or `fill`) on creation; `names` picks the tables that exist."""

    def __init__(self, device: int, n: int, names=QC_CLASSES, fill: Optional[np.ndarray] = None):
        self.device, self.n, self.names = device, int(n), tuple(names)
        fill = np.zeros(self.n, dtype=np.uint64) if fill is None else np.ascontiguousarray(fill, dtype=np.uint64)
        self.bufs = {name: DeviceBuffer.from_numpy(device, fill) for name in self.names}
        self.out = _abi.GenotypeSampleOut(*[self.bufs[k].ptr if k in self.bufs else None for k in QC_CLASSES + ("weighted_called",)])

    def tables(self) -> Dict[str, np.ndarray]:
        return {name: b.to_numpy(np.uint64, self.n) for name, b in self.bufs.items()}


def genotype_counts(m: DeviceMatrix, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
                    weights=None, site=QC_CLASSES, sample=QC_CLASSES, into: Optional[GenotypeSampleBuffers] = None, stream=None,
                    fill: Optional[int] = None) -> GenotypeCounts:
    """fmh_genotype_counts over rows [row_begin, row_begin + row_count) for the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all).  `site` / `sample`: the names of the tracks / tables to compute (empty or None: that side's pointer is NULL);
    `weights` [rows] uint32 adds the table weighted_called.  `keep` [rows] restricts the sample tables.  `into`: accumulate into these
    buffers.  `fill` pre-fills the site tracks with that byte (tests: the call must write every entry)."""
    rows = m.variants - row_begin if row_count is None else row_count
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.size != rows:
            raise ValueError("keep has one entry per row of the range")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.uint32)
        if weights.size != rows:
            raise ValueError("weights has one entry per row of the range")
    site, sample = tuple(site or ()), tuple(sample or ())
    tracks = {name: (DeviceBuffer(m.device, max(4 * rows, 4)) if fill is None else
                     DeviceBuffer.from_numpy(m.device, np.full(max(4 * rows, 4), fill, dtype=np.uint8))) for name in site}
    site_out = _abi.GenotypeSiteOut(*[tracks[k].ptr if k in tracks else None for k in QC_CLASSES])
    bufs = into
    if bufs is None and (sample or weights is not None):
        bufs = GenotypeSampleBuffers(m.device, n, sample + (("weighted_called",) if weights is not None else ()))
    kept = C.c_uint64(0)
    _abi.check(_abi.load().fmh_genotype_counts(m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), _ptr(weights), C.byref(site_out) if tracks else None,
                                               C.byref(bufs.out) if bufs is not None else None, C.byref(kept), stream))
    site_np = {name: t.to_numpy(np.uint32, rows) for name, t in tracks.items()} if tracks else None
    return GenotypeCounts(site_np, None if bufs is None else bufs.tables(), int(kept.value))


def hwe_exact(m_device: int, hom_ref, het, hom_alt, stream=None) -> np.ndarray:
    """fmh_hwe_exact: the exact-test p of every site on device `m_device` from the three uint32 count arrays."""
    arrays = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (hom_ref, het, hom_alt)]
    n = arrays[0].size
    if any(a.size != n for a in arrays):
        raise ValueError("the three count arrays have one entry per site")
    if n == 0:
        return np.zeros(0, dtype=np.float64)
    bufs = [DeviceBuffer.from_numpy(m_device, a) for a in arrays]
    d_p = DeviceBuffer(m_device, 8 * n)
    _abi.check(_abi.load().fmh_hwe_exact(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, d_p.ptr, m_device, stream))
    return d_p.to_numpy(np.float64, n)


def _site_counts(hom_ref, het, hom_alt):
    arrays = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (hom_ref, het, hom_alt)]
    if any(a.size != arrays[0].size for a in arrays):
        raise ValueError("the three count arrays have one entry per site")
    return arrays


def hwe_exact_host(hom_ref, het, hom_alt) -> np.ndarray:
    """fmh_hwe_exact_host (host only): the same function as the device's, on host arrays."""
    arrays = _site_counts(hom_ref, het, hom_alt)
    p = np.zeros(arrays[0].size, dtype=np.float64)
    _abi.check(_abi.load().fmh_hwe_exact_host(*[_ptr(a) for a in arrays], p.size, _ptr(p)))
    return p


def genotype_site_stats(hom_ref, het, hom_alt, n_samples: int) -> Dict[str, np.ndarray]:
    """fmh_genotype_site_stats (host only): call_rate, alt_frequency, maf, f_is and expected_het per site."""
    arrays = _site_counts(hom_ref, het, hom_alt)
    out = {name: np.zeros(arrays[0].size, dtype=np.float64) for name in QC_SITE_STATS}
    ptrs = _abi.GenotypeSiteStatsOut(*[out[name].ctypes.data for name in QC_SITE_STATS])
    _abi.check(_abi.load().fmh_genotype_site_stats(*[_ptr(a) for a in arrays], arrays[0].size, int(n_samples), C.byref(ptrs)))
    return out


def genotype_site_weights(hom_ref, het, hom_alt) -> np.ndarray:
    """fmh_genotype_site_weights (host only): w = rint(e * 2^31) per site, the row weights of the inbreeding coefficient."""
    arrays = _site_counts(hom_ref, het, hom_alt)
    w = np.zeros(arrays[0].size, dtype=np.uint32)
    _abi.check(_abi.load().fmh_genotype_site_weights(*[_ptr(a) for a in arrays], w.size, _ptr(w)))
    return w


def genotype_sample_stats(hom_ref, het, hom_alt, kept_rows: int, weighted_called=None) -> Dict[str, np.ndarray]:
    """fmh_genotype_sample_stats (host only): call_rate and het_rate per sample, and f when the weighted called sums are given."""
    arrays = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (hom_ref, het, hom_alt)]
    n = arrays[0].size
    weighted = None if weighted_called is None else np.ascontiguousarray(weighted_called, dtype=np.uint64).reshape(-1)
    if any(a.size != n for a in arrays) or (weighted is not None and weighted.size != n):
        raise ValueError("the tables have one entry per sample")
    names = QC_SAMPLE_STATS if weighted is not None else QC_SAMPLE_STATS[:2]
    out = {name: np.zeros(n, dtype=np.float64) for name in names}
    ptrs = _abi.GenotypeSampleStatsOut(*[out[name].ctypes.data if name in out else None for name in QC_SAMPLE_STATS])
    _abi.check(_abi.load().fmh_genotype_sample_stats(*[_ptr(a) for a in arrays], _ptr(weighted), n, int(kept_rows), C.byref(ptrs)))
    return out


# ---- association scan: exact fixed-point dosage sums, regression per site --------------------------------------------------------------
ASSOC_DEFAULT_ITEM_ROWS = 4096   # FMH_ASSOC_ITEM_ROWS unset
ASSOC_MAX_COLUMNS = 64
ASSOC_MAX_SAMPLES = 1 << 22
ASSOC_STATS = ("beta", "se", "t", "p")


@dataclass
class AssocSums:
    dosage: np.ndarray              # [row_count][K] int64
    called: Optional[np.ndarray]    # [row_count][K] int64, or None when the called sums were not asked for


@dataclass
class AssocPrepared:
    values: np.ndarray      # [n][K] int32: the c basis columns, then the P phenotypes
    exponent: np.ndarray    # [K] int32
    total: np.ndarray       # [K] int64
    yy: np.ndarray          # [P] float64
    n_basis: int            # c
    dropped: np.ndarray     # [c_in] bool


def assoc_sums(m: DeviceMatrix, values, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None,
               called: bool = True, stream=None, fill: Optional[int] = None) -> AssocSums:
    """fmh_assoc_sums over rows [row_begin, row_begin + row_count) for the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all): S = sum of dosage x values and, with `called`, C = sum of called x values, [rows][K] int64.  `values` is
    [n][K] int32.  `fill` pre-fills the outputs with that byte (tests: the call must write every entry)."""
    rows = m.variants - row_begin if row_count is None else row_count
    values = np.ascontiguousarray(values, dtype=np.int32)
    if values.ndim != 2:
        raise ValueError("values is [n][K]")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if values.shape[0] != n:
        raise ValueError("values has one row per selected sample")
    k = values.shape[1]
    nbytes = max(8 * rows * k, 8)

    def buffer():
        return DeviceBuffer(m.device, nbytes) if fill is None else DeviceBuffer.from_numpy(m.device, np.full(nbytes, fill, dtype=np.uint8))

    d_s = buffer()
    d_c = buffer() if called else None
    _abi.check(_abi.load().fmh_assoc_sums(m._h, _ptr(samples), n, row_begin, rows, _ptr(values), k, d_s.ptr, None if d_c is None else d_c.ptr, stream))
    return AssocSums(d_s.to_numpy(np.int64, rows * k).reshape(rows, k), None if d_c is None else d_c.to_numpy(np.int64, rows * k).reshape(rows, k))


def assoc_prepare(phenotypes, covariates=None) -> AssocPrepared:
    """fmh_assoc_prepare (host only): the centred, orthonormalised covariate basis and the residualised phenotypes as i32 fixed point."""
    y = np.ascontiguousarray(phenotypes, dtype=np.float64)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    if y.ndim != 2:
        raise ValueError("phenotypes is [n] or [n][P]")
    n, p = y.shape
    x = None
    c_in = 0
    if covariates is not None:
        x = np.ascontiguousarray(covariates, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] != n:
            raise ValueError("covariates is [n][c_in]")
        c_in = x.shape[1]
    values = np.zeros(max(n * (c_in + p), 1), dtype=np.int32)
    exponent = np.zeros(c_in + p, dtype=np.int32)
    total = np.zeros(c_in + p, dtype=np.int64)
    yy = np.zeros(p, dtype=np.float64)
    dropped = np.zeros(max(c_in, 1), dtype=np.uint8)
    c = C.c_size_t(0)
    _abi.check(_abi.load().fmh_assoc_prepare(_ptr(y), None if c_in == 0 else _ptr(x), n, p, c_in, _ptr(values), _ptr(exponent), _ptr(total), _ptr(yy),
                                             C.byref(c), _ptr(dropped)))
    k = int(c.value) + p
    return AssocPrepared(values[: n * k].reshape(n, k).copy(), exponent[:k].copy(), total[:k].copy(), yy, int(c.value), dropped[:c_in].astype(bool))


def assoc_stats(dosage_sum, called_sum, hom_ref, het, hom_alt, total, exponent, yy, n_samples: int, n_basis: int,
                outputs=ASSOC_STATS) -> Dict[str, np.ndarray]:
    """fmh_assoc_stats (host only): beta, se, t and p [rows][P] from the sums, the QC tracks and fmh_assoc_prepare's T, e and yy."""
    s = np.ascontiguousarray(dosage_sum, dtype=np.int64)
    cs = np.ascontiguousarray(called_sum, dtype=np.int64)
    tracks = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (hom_ref, het, hom_alt)]
    yy = np.ascontiguousarray(yy, dtype=np.float64).reshape(-1)
    total = np.ascontiguousarray(total, dtype=np.int64).reshape(-1)
    exponent = np.ascontiguousarray(exponent, dtype=np.int32).reshape(-1)
    rows, p, k = tracks[0].size, yy.size, int(n_basis) + yy.size
    if s.size != rows * k or cs.size != rows * k or total.size != k or exponent.size != k or any(a.size != rows for a in tracks):
        raise ValueError("the sums are [rows][c + P], the tracks [rows], total and exponent [c + P]")
    out = {name: np.zeros((rows, p), dtype=np.float64) for name in outputs}
    _abi.check(_abi.load().fmh_assoc_stats(_ptr(s), _ptr(cs), *[_ptr(a) for a in tracks], rows, _ptr(total), _ptr(exponent), _ptr(yy), int(n_samples),
                                           int(n_basis), p, *[_ptr(out[name]) if name in out else None for name in ASSOC_STATS]))
    return out


# ---- polygenic scores: exact per-sample weighted dosage sums ----------------------------------------------------------------------------
SCORE_DEFAULT_ITEM_ROWS = 4096   # FMH_SCORE_ITEM_ROWS unset
SCORE_MAX_COLUMNS = 64
SCORE_MAX_ROWS = 1 << 21
SCORE_MODES = ("mean", "center", "zero")   # FMH_SCORE_MEAN, FMH_SCORE_CENTER, FMH_SCORE_ZERO


@dataclass
class ScoreSums:
    dosage: np.ndarray              # [n][K] int64
    called: Optional[np.ndarray]    # [n][K] int64, or None when the called sums were not asked for


@dataclass
class ScoreValues:
    dosage: np.ndarray              # V [rows][K] int32
    called: Optional[np.ndarray]    # U [rows][K] int32, or None without the site tracks
    called_total: Optional[np.ndarray]   # T_U [K] int64
    row_used: np.ndarray            # [rows] bool


def score_sums(m: DeviceMatrix, values, called_values=None, samples=None, n_samples: Optional[int] = None, row_begin: int = 0,
               row_count: Optional[int] = None, stream=None, fill: Optional[int] = None) -> ScoreSums:
    """fmh_score_sums over rows [row_begin, row_begin + row_count) for the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all): S = sum over rows of dosage x values and, with `called_values`, C = sum of called x called_values, [n][K]
    int64.  `values` and `called_values` are [rows][K] int32.  `fill` pre-fills the outputs with that byte (tests: the call must write every
    entry)."""
    rows = m.variants - row_begin if row_count is None else row_count
    values = np.ascontiguousarray(values, dtype=np.int32)
    if values.ndim != 2 or values.shape[0] != rows:
        raise ValueError("values is [rows][K], one row per row of the range")
    k = values.shape[1]
    if called_values is not None:
        called_values = np.ascontiguousarray(called_values, dtype=np.int32)
        if called_values.shape != values.shape:
            raise ValueError("called_values has the shape of values")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    nbytes = max(8 * n * k, 8)

    def buffer():
        return DeviceBuffer(m.device, nbytes) if fill is None else DeviceBuffer.from_numpy(m.device, np.full(nbytes, fill, dtype=np.uint8))

    d_s = buffer()
    d_c = buffer() if called_values is not None else None
    _abi.check(_abi.load().fmh_score_sums(m._h, _ptr(samples), n, row_begin, rows, _ptr(values), _ptr(called_values), k, d_s.ptr,
                                          None if d_c is None else d_c.ptr, stream))
    return ScoreSums(d_s.to_numpy(np.int64, n * k).reshape(n, k), None if d_c is None else d_c.to_numpy(np.int64, n * k).reshape(n, k))


def _score_weights(weights) -> np.ndarray:
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    if w.ndim != 2:
        raise ValueError("weights is [rows] or [rows][K]")
    return w


def score_exponents(weights) -> np.ndarray:
    """fmh_score_exponents (host only): per weight column the largest e with 2 max|w| 2^e <= 2^30; int32 [K]."""
    w = _score_weights(weights)
    e = np.zeros(max(w.shape[1], 1), dtype=np.int32)
    _abi.check(_abi.load().fmh_score_exponents(_ptr(w), w.shape[0], w.shape[1], _ptr(e)))
    return e[: w.shape[1]]


def score_values(weights, exponents, hom_ref=None, het=None, hom_alt=None, called: Optional[bool] = None) -> ScoreValues:
    """fmh_score_values (host only): V = rint(w 2^e) and, with the three site tracks, U = rint((mu w) 2^e) with its exact column totals;
    which rows are used.  `called`: whether U is wanted (default: whenever the tracks are given)."""
    w = _score_weights(weights)
    rows, k = w.shape
    e = np.ascontiguousarray(exponents, dtype=np.int32).reshape(-1)
    if e.size != k:
        raise ValueError("one exponent per weight column")
    tracks = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (hom_ref, het, hom_alt)]
    if any(a is not None and a.size != rows for a in tracks):
        raise ValueError("the tracks have one entry per row")
    want_u = all(a is not None for a in tracks) if called is None else bool(called)
    v = np.zeros((rows, k), dtype=np.int32)
    u = np.zeros((rows, k), dtype=np.int32) if want_u else None
    total = np.zeros(k, dtype=np.int64) if want_u else None
    used = np.zeros(max(rows, 1), dtype=np.uint8)
    _abi.check(_abi.load().fmh_score_values(_ptr(w), rows, k, _ptr(e), *[_ptr(a) for a in tracks], _ptr(v), _ptr(u), _ptr(total), _ptr(used)))
    return ScoreValues(v, u, total, used[:rows].astype(bool))


def score_stats(dosage_sum, exponents, called_sum=None, called_total=None, mode: str = "mean") -> np.ndarray:
    """fmh_score_stats (host only): the scores f64 [n][K] from the exact sums, mode "mean", "center" or "zero"."""
    s = np.ascontiguousarray(dosage_sum, dtype=np.int64)
    e = np.ascontiguousarray(exponents, dtype=np.int32).reshape(-1)
    if s.ndim != 2 or s.shape[1] != e.size:
        raise ValueError("dosage_sum is [n][K], exponents [K]")
    c = None if called_sum is None else np.ascontiguousarray(called_sum, dtype=np.int64)
    t = None if called_total is None else np.ascontiguousarray(called_total, dtype=np.int64).reshape(-1)
    if (c is not None and c.shape != s.shape) or (t is not None and t.size != e.size):
        raise ValueError("called_sum is [n][K], called_total [K]")
    out = np.zeros(s.shape, dtype=np.float64)
    _abi.check(_abi.load().fmh_score_stats(_ptr(s), _ptr(c), _ptr(t), _ptr(e), s.shape[0], s.shape[1], SCORE_MODES.index(mode), _ptr(out)))
    return out


# ---- logistic association scan: score test from exact class sums ------------------------------------------------------------------------
LOGISTIC_MAX_SAMPLES = 1 << 21
LOGISTIC_STATS = ("chi2", "z", "p", "beta", "se")
LOGISTIC_REASONS = ("fitted", "one_class", "not_converged", "pivot", "zero_weight", "basis_lost")   # FMH_LOGISTIC_* 0 .. 5


@dataclass
class LogisticNull:
    values: List[np.ndarray]   # per phenotype batch [n][Pb * (c + 3)] int32: what one fmh_assoc_sums call takes
    exponent: np.ndarray       # [P][c + 3] int32
    total: np.ndarray          # [P][c + 3] int64
    fitted: np.ndarray         # [P] bool
    reason: np.ndarray         # [P] int32 (FMH_LOGISTIC_*)
    iterations: np.ndarray     # [P] int32
    n_cases: np.ndarray        # [P] uint64
    n_basis: int               # c
    dropped: np.ndarray        # [c_in] bool
    batch: int                 # floor(64 / (c + 3)) phenotypes per batch


def assoc_homalt_sums(m: DeviceMatrix, values, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None,
                      stream=None, fill: Optional[int] = None) -> np.ndarray:
    """fmh_assoc_homalt_sums over rows [row_begin, row_begin + row_count): H = sum over the called hom-alt genotypes of the selected samples
    of values, [rows][K] int64.  `values` is [n][K] int32.  `fill` pre-fills the output with that byte (tests: every entry is written)."""
    rows = m.variants - row_begin if row_count is None else row_count
    values = np.ascontiguousarray(values, dtype=np.int32)
    if values.ndim != 2:
        raise ValueError("values is [n][K]")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if values.shape[0] != n:
        raise ValueError("values has one row per selected sample")
    k = values.shape[1]
    nbytes = max(8 * rows * k, 8)
    d_h = DeviceBuffer(m.device, nbytes) if fill is None else DeviceBuffer.from_numpy(m.device, np.full(nbytes, fill, dtype=np.uint8))
    _abi.check(_abi.load().fmh_assoc_homalt_sums(m._h, _ptr(samples), n, row_begin, rows, _ptr(values), k, d_h.ptr, stream))
    return d_h.to_numpy(np.int64, rows * k).reshape(rows, k)


def logistic_null(phenotypes, covariates=None) -> LogisticNull:
    """fmh_logistic_null (host only): the null model of every case / control phenotype and its c + 3 value columns as i32 fixed point."""
    y = np.ascontiguousarray(phenotypes, dtype=np.float64)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    if y.ndim != 2:
        raise ValueError("phenotypes is [n] or [n][P]")
    n, p = y.shape
    x = None
    c_in = 0
    if covariates is not None:
        x = np.ascontiguousarray(covariates, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] != n:
            raise ValueError("covariates is [n][c_in]")
        c_in = x.shape[1]
    values = np.zeros(max(n * p * (c_in + 3), 1), dtype=np.int32)
    exponent = np.zeros(max(p * (c_in + 3), 1), dtype=np.int32)
    total = np.zeros(max(p * (c_in + 3), 1), dtype=np.int64)
    fitted, reason, iterations = np.zeros(max(p, 1), np.uint8), np.zeros(max(p, 1), np.int32), np.zeros(max(p, 1), np.int32)
    n_cases = np.zeros(max(p, 1), dtype=np.uint64)
    dropped = np.zeros(max(c_in, 1), dtype=np.uint8)
    c = C.c_size_t(0)
    _abi.check(_abi.load().fmh_logistic_null(_ptr(y), None if c_in == 0 else _ptr(x), n, p, c_in, _ptr(values), _ptr(exponent), _ptr(total), _ptr(fitted),
                                             _ptr(reason), _ptr(iterations), _ptr(n_cases), C.byref(c), _ptr(dropped)))
    w = int(c.value) + 3
    batch = ASSOC_MAX_COLUMNS // w
    tables = []
    for first in range(0, p, batch):
        pb = min(batch, p - first)
        tables.append(values[n * w * first: n * w * (first + pb)].reshape(n, pb * w).copy())
    return LogisticNull(tables, exponent[: p * w].reshape(p, w).copy(), total[: p * w].reshape(p, w).copy(), fitted[:p].astype(bool), reason[:p].copy(),
                        iterations[:p].copy(), n_cases[:p].copy(), int(c.value), dropped[:c_in].astype(bool), batch)


def _logistic_score_inputs(dosage_sum, called_sum, homalt_sum, hom_ref, het, hom_alt, total, exponent, n_basis):
    h = np.ascontiguousarray(homalt_sum, dtype=np.int64)
    tracks = [np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (hom_ref, het, hom_alt)]
    rows = tracks[0].size
    pb = h.size // rows if rows else (h.shape[1] if h.ndim == 2 else 1)
    k = pb * (int(n_basis) + 3)
    s = np.ascontiguousarray(dosage_sum, dtype=np.int64)
    cs = np.ascontiguousarray(called_sum, dtype=np.int64)
    total = np.ascontiguousarray(total, dtype=np.int64).reshape(-1)
    exponent = np.ascontiguousarray(exponent, dtype=np.int32).reshape(-1)
    if s.size != rows * k or cs.size != rows * k or h.size != rows * pb or total.size != k or exponent.size != k or any(a.size != rows for a in tracks):
        raise ValueError("the sums are [rows][Pb * (c + 3)], the hom-alt sums [rows][Pb], the tracks [rows], total and exponent [Pb * (c + 3)]")
    return s, cs, h, tracks, total, exponent, rows, pb


def logistic_score_host(dosage_sum, called_sum, homalt_sum, hom_ref, het, hom_alt, total, exponent, n_basis: int):
    """fmh_logistic_score_host (host only): (score, variance), each [rows][Pb] float64, of one phenotype batch."""
    s, cs, h, tracks, total, exponent, rows, pb = _logistic_score_inputs(dosage_sum, called_sum, homalt_sum, hom_ref, het, hom_alt, total, exponent, n_basis)
    score, variance = np.zeros((rows, pb)), np.zeros((rows, pb))
    _abi.check(_abi.load().fmh_logistic_score_host(_ptr(s), _ptr(cs), _ptr(h), *[_ptr(a) for a in tracks], rows, _ptr(total), _ptr(exponent), int(n_basis),
                                                   pb, _ptr(score), _ptr(variance)))
    return score, variance


def logistic_score(device: int, dosage_sum, called_sum, homalt_sum, hom_ref, het, hom_alt, total, exponent, n_basis: int, stream=None,
                   fill: Optional[int] = None):
    """fmh_logistic_score on device `device`: the same function as the host twin's, from device copies of the host arrays given."""
    s, cs, h, tracks, total, exponent, rows, pb = _logistic_score_inputs(dosage_sum, called_sum, homalt_sum, hom_ref, het, hom_alt, total, exponent, n_basis)
    if rows == 0:
        return np.zeros((0, pb)), np.zeros((0, pb))
    bufs = [DeviceBuffer.from_numpy(device, a) for a in (s, cs, h, *tracks)]
    nbytes = 8 * rows * pb
    out = [DeviceBuffer(device, nbytes) if fill is None else DeviceBuffer.from_numpy(device, np.full(nbytes, fill, dtype=np.uint8)) for _ in range(2)]
    _abi.check(_abi.load().fmh_logistic_score(*[b.ptr for b in bufs], rows, _ptr(total), _ptr(exponent), int(n_basis), pb, out[0].ptr, out[1].ptr, device,
                                              stream))
    return tuple(o.to_numpy(np.float64, rows * pb).reshape(rows, pb) for o in out)


def logistic_stats(score, variance, outputs=LOGISTIC_STATS) -> Dict[str, np.ndarray]:
    """fmh_logistic_stats (host only): chi2, z, p, beta and se, shaped as `score`."""
    u = np.ascontiguousarray(score, dtype=np.float64)
    v = np.ascontiguousarray(variance, dtype=np.float64)
    if u.shape != v.shape:
        raise ValueError("score and variance have one shape")
    out = {name: np.zeros(u.shape, dtype=np.float64) for name in outputs}
    _abi.check(_abi.load().fmh_logistic_stats(_ptr(u), _ptr(v), u.size, *[_ptr(out[name]) if name in out else None for name in LOGISTIC_STATS]))
    return out


# ---- what the segment statistics (runs of homozygosity, IBD segments) share --------------------------------------------------------------------
def _scan_range(m, samples, n_samples, row_begin, row_count, keep, positions):
    """The arguments of a device scan as the library takes them: (samples, n, rows of the range, keep, positions)."""
    rows = m.variants - row_begin if row_count is None else row_count
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.size != rows:
            raise ValueError("keep has one entry per row of the range")
    if positions is not None:
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        if positions.size != m.variants:
            raise ValueError("positions has one entry per row of the matrix")
    return samples, n, rows, keep, positions


def _kept_positions(x, K):
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if x.size != K:
            raise ValueError("x has one entry per kept row")
    return x


def _segment_scan(call, sizes: Dict[str, int], dtype: np.dtype, capacity: Optional[int], device: Optional[int] = None):
    """One fmh_*_scan (device None: fmh_*_scan_host, on host arrays).  call(pointers, segments, capacity, count) gets {table: pointer} for
    uint64 tables of `sizes` elements, pre-filled with junk, a buffer of `capacity` segments (0: they are counted only, None: not even that)
    and the count's reference.  Returns ({table: flat array}, segments [min(count, capacity)] or None, count or None)."""
    host = device is None
    bufs = {name: np.full(max(size, 1), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64) for name, size in sizes.items()}
    seg = np.zeros(capacity, dtype=dtype) if capacity else None
    if not host:
        bufs = {name: DeviceBuffer.from_numpy(device, junk) for name, junk in bufs.items()}
        seg = DeviceBuffer(device, capacity * dtype.itemsize) if capacity else None
    count = C.c_uint64(0)
    call({name: b.ctypes.data if host else b.ptr for name, b in bufs.items()}, None if seg is None else _ptr(seg) if host else seg.ptr, capacity or 0,
         C.byref(count) if capacity is not None else None)
    tables = {name: bufs[name][:size].copy() if host else bufs[name].to_numpy(np.uint64, size) for name, size in sizes.items()}
    if capacity is None:
        return tables, None, None
    stored = min(int(count.value), capacity)
    segments = np.zeros(0, dtype=dtype) if seg is None else seg[:stored].copy() if host else seg.to_numpy(dtype, stored)
    return tables, segments, int(count.value)


def _sort_segments(sort, segments, dtype: np.dtype) -> np.ndarray:
    out = np.ascontiguousarray(segments, dtype=dtype).copy()
    _abi.check(sort(_ptr(out) if out.size else None, out.size))
    return out


# ---- runs of homozygosity: per-sample sliding-window scan along the kept rows ---------------------------------------------------------------
ROH_DEFAULT_ITEM_ROWS = 4096   # FMH_ROH_ITEM_ROWS unset
ROH_TABLES = ("n_runs", "sum_sites", "sum_length", "longest_length")
ROH_SEGMENT_DTYPE = np.dtype([("sample", np.uint32), ("n_sites", np.uint32), ("n_het", np.uint32), ("n_missing", np.uint32),
                              ("first_row", np.uint64), ("last_row", np.uint64)])
ROH_NO_LIMIT = 0xFFFFFFFF


def roh_need(threshold: float, window: int) -> np.ndarray:
    """fmh_roh_need (host only): need[65], need[c] for c = 1..window the smallest h >= 1 with h >= threshold * c."""
    need = np.zeros(65, dtype=np.uint8)
    _abi.check(_abi.load().fmh_roh_need(float(threshold), int(window), _ptr(need)))
    return need


def roh_params(window=50, window_het=1, window_missing=5, threshold=0.05, need=None, min_sites=100, min_length=1_000_000, max_gap=1_000_000,
               max_bp_per_site=50_000, max_het=None, max_missing=None, bin_edges=()) -> "_abi.RohParams":
    """fmh_roh_params with PLINK's defaults; `need` overrides the table of `threshold`; len(bin_edges) + 1 bins when edges are given
    (bin_edges=None or (): no bins; n_bins may also be set on the result)."""
    p = _abi.RohParams()
    p.window, p.window_het, p.window_missing = int(window), int(window_het), int(window_missing)
    table = roh_need(threshold, window) if need is None else np.ascontiguousarray(need, dtype=np.uint8)
    for c in range(65):
        p.need[c] = int(table[c])
    p.min_sites, p.min_length, p.max_gap, p.max_bp_per_site = int(min_sites), int(min_length), int(max_gap or 0), int(max_bp_per_site or 0)
    p.max_het = ROH_NO_LIMIT if max_het is None else int(max_het)
    p.max_missing = ROH_NO_LIMIT if max_missing is None else int(max_missing)
    edges = list(bin_edges or ())
    p.n_bins = len(edges) + 1 if edges else 0
    for b, e in enumerate(edges[:7]):
        p.bin_edges[b] = int(e)
    return p


@dataclass
class RohResult:
    tables: Dict[str, np.ndarray]        # n_runs, sum_sites, sum_length, longest_length: [n] uint64; bin_runs, bin_length: [n][n_bins]
    segments: Optional[np.ndarray]       # ROH_SEGMENT_DTYPE [min(count, capacity)], in the order they were stored, or None
    count: Optional[int]                 # the exact number of qualifying runs, or None when segments were not asked for


def _roh_scan(call, n, n_bins, capacity, device=None) -> RohResult:
    sizes = {name: n for name in ROH_TABLES}
    sizes.update(bin_runs=n * n_bins, bin_length=n * n_bins)
    tables, segments, count = _segment_scan(lambda ptrs, *rest: call(_abi.RohOut(*[ptrs[name] for name in sizes]), *rest), sizes,
                                            ROH_SEGMENT_DTYPE, capacity, device)
    for name in ("bin_runs", "bin_length"):
        tables[name] = tables[name].reshape(n, n_bins)
    return RohResult(tables, segments, count)


def roh_scan(m: DeviceMatrix, params, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
             positions=None, capacity: Optional[int] = None, stream=None) -> RohResult:
    """fmh_roh_scan over rows [row_begin, row_begin + row_count) for the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all).  `positions` [variants] uint32 (indexed by matrix row) or None.  `capacity`: None = no segments, else the
    elements of the segment buffer (0: the runs are counted only)."""
    samples, n, rows, keep, positions = _scan_range(m, samples, n_samples, row_begin, row_count, keep, positions)
    return _roh_scan(lambda out, seg, cap, count: _abi.check(_abi.load().fmh_roh_scan(
        m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), _ptr(positions), C.byref(params), C.byref(out), seg, cap, count, stream)),
        n, int(params.n_bins), capacity, m.device)


def roh_scan_host(state, params, x=None, capacity: Optional[int] = None) -> RohResult:
    """fmh_roh_scan_host (host only): the same scan over `state` uint8 [K][n] (0 HOM, 1 HET, 2 MISS) and `x` uint32 [K] or None."""
    state = np.ascontiguousarray(state, dtype=np.uint8)
    K, n = state.shape
    x = _kept_positions(x, K)
    return _roh_scan(lambda out, seg, cap, count: _abi.check(_abi.load().fmh_roh_scan_host(
        _ptr(state) if state.size else None, _ptr(x), K, n, C.byref(params), C.byref(out), seg, cap, count)), n, int(params.n_bins), capacity)


def roh_sort_segments(segments: np.ndarray) -> np.ndarray:
    """fmh_roh_sort_segments (host only): a copy ordered by (sample, first_row)."""
    return _sort_segments(_abi.load().fmh_roh_sort_segments, segments, ROH_SEGMENT_DTYPE)


# ---- IBD segments: pairwise shared-segment scan along the kept rows ----------------------------------------------------------------------------
IBD1, IBD2 = 1, 2
IBD_TABLES = ("n_segments", "sum_sites", "sum_length", "longest_length")
IBD_SEGMENT_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("n_sites", np.uint32), ("n_missing", np.uint32),
                              ("first_row", np.uint64), ("last_row", np.uint64)])
IBD_NO_LIMIT = 0xFFFFFFFF


def ibd_params(mode=IBD1, min_sites=436, min_length=7_000_000, max_gap=1_000_000, max_bp_per_site=0, max_missing=None) -> "_abi.IbdParams":
    """fmh_ibd_params with IBIS's defaults (7 cM read at 1 cM per Mb, 436 markers); mode is IBD1, IBD2, "ibd1" or "ibd2"."""
    p = _abi.IbdParams()
    p.mode = {"ibd1": IBD1, "ibd2": IBD2}.get(mode, mode) if isinstance(mode, str) else int(mode)
    p.min_sites, p.min_length, p.max_gap, p.max_bp_per_site = int(min_sites), int(min_length), int(max_gap or 0), int(max_bp_per_site or 0)
    p.max_missing = IBD_NO_LIMIT if max_missing is None else int(max_missing)
    return p


@dataclass
class IbdResult:
    tables: Dict[str, np.ndarray]        # n_segments, sum_sites, sum_length, longest_length: [n][n] uint64
    segments: Optional[np.ndarray]       # IBD_SEGMENT_DTYPE [min(count, capacity)], in the order they were stored, or None
    count: Optional[int]                 # the exact number of qualifying runs, or None when segments were not asked for


def _ibd_scan(call, n, names, capacity, device=None) -> IbdResult:
    """`names`: the tables asked for; the others go to the library as NULL."""
    tables, segments, count = _segment_scan(lambda ptrs, *rest: call(_abi.IbdOut(*[ptrs.get(name) for name in IBD_TABLES]), *rest),
                                            {name: n * n for name in names}, IBD_SEGMENT_DTYPE, capacity, device)
    return IbdResult({name: t.reshape(n, n) for name, t in tables.items()}, segments, count)


def ibd_scan(m: DeviceMatrix, params, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
             positions=None, capacity: Optional[int] = None, stream=None, tables=IBD_TABLES) -> IbdResult:
    """fmh_ibd_scan over rows [row_begin, row_begin + row_count) for all pairs of the samples `samples` (ascending sample numbers; None = the
    first n_samples, default all).  `positions` [variants] uint32 (indexed by matrix row) or None.  `capacity`: None = no segments, else the
    elements of the segment buffer (0: the runs are counted only).  `tables`: the tables asked for; they are pre-filled with junk."""
    samples, n, rows, keep, positions = _scan_range(m, samples, n_samples, row_begin, row_count, keep, positions)
    return _ibd_scan(lambda out, seg, cap, count: _abi.check(_abi.load().fmh_ibd_scan(
        m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), _ptr(positions), C.byref(params), C.byref(out) if tables else None, seg, cap, count, stream)),
        n, tables, capacity, m.device)


def ibd_scan_host(dosage, params, x=None, capacity: Optional[int] = None) -> IbdResult:
    """fmh_ibd_scan_host (host only): the same scan over `dosage` uint8 [K][n] (0, 1, 2; 3 = not called) and `x` uint32 [K] or None."""
    dosage = np.ascontiguousarray(dosage, dtype=np.uint8)
    K, n = dosage.shape
    x = _kept_positions(x, K)
    return _ibd_scan(lambda out, seg, cap, count: _abi.check(_abi.load().fmh_ibd_scan_host(
        _ptr(dosage) if dosage.size else None, _ptr(x), K, n, C.byref(params), C.byref(out), seg, cap, count)), n, IBD_TABLES, capacity)


def ibd_sort_segments(segments: np.ndarray) -> np.ndarray:
    """fmh_ibd_sort_segments (host only): a copy ordered by (a, b, first_row)."""
    return _sort_segments(_abi.load().fmh_ibd_sort_segments, segments, IBD_SEGMENT_DTYPE)


# ---- LD clumping: genotype r^2 around index sites --------------------------------------------------------------------------------------------
CLUMP_NONE = 0xFFFFFFFF
GENO_LD_COUNTS = ("n", "sum_a", "sum_b", "sq_a", "sq_b", "cross")


def clump_params(p1=1e-4, p2=1e-2, r2=0.5, window=250_000) -> "_abi.ClumpParams":
    """fmh_clump_params with PLINK's --clump defaults (window in position units)."""
    p = _abi.ClumpParams()
    p.p1, p.p2, p.r2, p.window, p.reserved = float(p1), float(p2), float(r2), int(window), 0
    return p


@dataclass
class ClumpResult:
    index_of: np.ndarray     # uint32 [rows]: the index's row (relative to row_begin), CLUMP_NONE for a row in no clump
    r2: Optional[np.ndarray]  # float64 [rows]: r^2 with the index, NaN for a row in no clump
    n_clumps: int


def clump(m: DeviceMatrix, p_values, params, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None,
          keep=None, positions=None, want_r2: bool = True, stream=None) -> ClumpResult:
    """fmh_clump over rows [row_begin, row_begin + row_count) and the samples `samples` (ascending sample numbers; None = the first n_samples,
    default all).  `p_values` float64 [row_count]; `positions` [variants] uint32 (indexed by matrix row) or None.  The outputs are pre-filled
    with junk."""
    rows = m.variants - row_begin if row_count is None else row_count
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    p_values = np.ascontiguousarray(p_values, dtype=np.float64)
    if p_values.size != rows:
        raise ValueError("p_values has one entry per row of the range")
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.size != rows:
            raise ValueError("keep has one entry per row of the range")
    if positions is not None:
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        if positions.size != m.variants:
            raise ValueError("positions has one entry per row of the matrix")
    index_of = np.full(max(rows, 1), 0xA5A5A5A5, dtype=np.uint32)
    r2 = np.full(max(rows, 1), 12345.678, dtype=np.float64) if want_r2 else None
    count = C.c_uint64(0xA5A5A5A5)
    _abi.check(_abi.load().fmh_clump(m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), _ptr(positions), _ptr(p_values),
                                     C.byref(params), _ptr(index_of), _ptr(r2), C.byref(count), stream))
    return ClumpResult(index_of[:rows], None if r2 is None else r2[:rows], int(count.value))


def clump_host(dosage, p_values, params, x=None, want_r2: bool = True) -> ClumpResult:
    """fmh_clump_host (host only): the same rule over `dosage` uint8 [K][n] (0, 1, 2; 3 = not called), `x` uint32 [K] or None."""
    dosage = np.ascontiguousarray(dosage, dtype=np.uint8)
    K, n = dosage.shape
    p_values = np.ascontiguousarray(p_values, dtype=np.float64)
    if p_values.size != K:
        raise ValueError("p_values has one entry per row")
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if x.size != K:
            raise ValueError("x has one entry per row")
    index_of = np.full(max(K, 1), 0xA5A5A5A5, dtype=np.uint32)
    r2 = np.full(max(K, 1), 12345.678, dtype=np.float64) if want_r2 else None
    count = C.c_uint64(0xA5A5A5A5)
    _abi.check(_abi.load().fmh_clump_host(_ptr(dosage) if dosage.size else None, _ptr(x), _ptr(p_values) if K else None, K, n, C.byref(params),
                                          _ptr(index_of), _ptr(r2), C.byref(count)))
    return ClumpResult(index_of[:K], None if r2 is None else r2[:K], int(count.value))


def _count_table(records: np.ndarray) -> np.ndarray:
    return records.reshape(-1, 8)[:, :6].astype(np.int64)


def geno_ld_pairs(m: DeviceMatrix, rows_a, rows_b, samples=None, n_samples: Optional[int] = None, stream=None) -> np.ndarray:
    """fmh_geno_ld_pairs: int64 [P][6] (GENO_LD_COUNTS) of the pairs of matrix rows; the device records are pre-filled with junk."""
    rows_a = np.ascontiguousarray(rows_a, dtype=np.uint32)
    rows_b = np.ascontiguousarray(rows_b, dtype=np.uint32)
    if rows_a.shape != rows_b.shape or rows_a.ndim != 1:
        raise ValueError("rows_a and rows_b are one-dimensional and of one length")
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    P = rows_a.size
    buf = DeviceBuffer.from_numpy(m.device, np.full(max(P, 1) * 8, 0xA5A5A5A5, dtype=np.uint32))
    _abi.check(_abi.load().fmh_geno_ld_pairs(m._h, _ptr(samples), n, _ptr(rows_a) if P else None, _ptr(rows_b) if P else None, P, buf.ptr if P else None, stream))
    records = buf.to_numpy(np.uint32, max(P, 1) * 8)[: P * 8]
    if P and records.reshape(-1, 8)[:, 6:].any():
        raise AssertionError("the reserved words of a record are not 0")
    return _count_table(records)


def geno_ld_pairs_host(dosage, rows_a, rows_b) -> np.ndarray:
    """fmh_geno_ld_pairs_host (host only): int64 [P][6] of pairs of rows of `dosage` uint8 [K][n]."""
    dosage = np.ascontiguousarray(dosage, dtype=np.uint8)
    K, n = dosage.shape
    rows_a = np.ascontiguousarray(rows_a, dtype=np.uint32)
    rows_b = np.ascontiguousarray(rows_b, dtype=np.uint32)
    P = rows_a.size
    records = np.full(max(P, 1) * 8, 0xA5A5A5A5, dtype=np.uint32)
    _abi.check(_abi.load().fmh_geno_ld_pairs_host(_ptr(dosage) if dosage.size else None, K, n, _ptr(rows_a) if P else None, _ptr(rows_b) if P else None, P,
                                                  _ptr(records) if P else None))
    return _count_table(records[: P * 8])


def geno_ld_r2(counts) -> np.ndarray:
    """fmh_geno_ld_r2 (host only): float64 [P] of int [P][6] counts (GENO_LD_COUNTS) by the definition's one formula."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 6)
    P = counts.shape[0]
    records = np.zeros((max(P, 1), 8), dtype=np.uint32)
    records[:P, :6] = counts
    out = np.full(max(P, 1), 12345.678, dtype=np.float64)
    _abi.check(_abi.load().fmh_geno_ld_r2(_ptr(records) if P else None, P, _ptr(out) if P else None))
    return out[:P]


# ---- LD scores and LD score regression ---------------------------------------------------------------------------------------------------------
LDSCORE_ADJUST = 1
LDSCORE_ROW_BYTES, LDSCORE_ITEM_BYTES, LDSCORE_TILE = 28, 8, 64   # FMH_LDSCORE_BUDGET_BYTES counts these; an item is a pair of 64-row tiles
LDSC_OUT = ("h2", "h2_se", "intercept", "intercept_se", "ratio", "mean_chi2", "lambda_gc", "n_used", "blocks")


def ldscore_params(window=1_000_000, adjust=True) -> "_abi.LdScoreParams":
    """fmh_ldscore_params (window in position units; adjust = ldsc's bias correction of every r^2)."""
    p = _abi.LdScoreParams()
    p.window, p.flags = int(window), LDSCORE_ADJUST if adjust else 0
    return p


@dataclass
class LdScoreSums:
    q: np.ndarray          # int64 [rows]: the sum of the pair terms in units of 2^-40
    partners: Optional[np.ndarray]  # uint32 [rows]: kept rows within the window
    counted: np.ndarray    # uint32 [rows]: those whose term is defined


def ld_scores(m: DeviceMatrix, params, samples=None, n_samples: Optional[int] = None, row_begin: int = 0, row_count: Optional[int] = None, keep=None,
              positions=None, want_partners: bool = True, stream=None) -> LdScoreSums:
    """fmh_ld_scores over rows [row_begin, row_begin + row_count) and the samples `samples` (ascending sample numbers; None = the first
    n_samples, default all).  `positions` [variants] uint32 (indexed by matrix row) or None.  The outputs are pre-filled with junk."""
    rows = m.variants - row_begin if row_count is None else row_count
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = samples.size
    else:
        n = m.samples if n_samples is None else int(n_samples)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.size != rows:
            raise ValueError("keep has one entry per row of the range")
    if positions is not None:
        positions = np.ascontiguousarray(positions, dtype=np.uint32)
        if positions.size != m.variants:
            raise ValueError("positions has one entry per row of the matrix")
    q = np.full(max(rows, 1), -0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    partners = np.full(max(rows, 1), 0xA5A5A5A5, dtype=np.uint32) if want_partners else None
    counted = np.full(max(rows, 1), 0xA5A5A5A5, dtype=np.uint32)
    _abi.check(_abi.load().fmh_ld_scores(m._h, _ptr(samples), n, row_begin, rows, _ptr(keep), _ptr(positions), C.byref(params), _ptr(q), _ptr(partners),
                                         _ptr(counted), stream))
    return LdScoreSums(q[:rows], None if partners is None else partners[:rows], counted[:rows])


def ld_scores_host(dosage, params, x=None, want_partners: bool = True) -> LdScoreSums:
    """fmh_ld_scores_host (host only): the same rule over `dosage` uint8 [K][n] (0, 1, 2; 3 = not called), `x` uint32 [K] or None."""
    dosage = np.ascontiguousarray(dosage, dtype=np.uint8)
    K, n = dosage.shape
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if x.size != K:
            raise ValueError("x has one entry per row")
    q = np.full(max(K, 1), -0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    partners = np.full(max(K, 1), 0xA5A5A5A5, dtype=np.uint32) if want_partners else None
    counted = np.full(max(K, 1), 0xA5A5A5A5, dtype=np.uint32)
    _abi.check(_abi.load().fmh_ld_scores_host(_ptr(dosage) if dosage.size else None, _ptr(x), K, n, C.byref(params), _ptr(q), _ptr(partners), _ptr(counted)))
    return LdScoreSums(q[:K], None if partners is None else partners[:K], counted[:K])


def ld_score_values(q, counted) -> np.ndarray:
    """fmh_ld_score_values (host only): float64 [K] = q * 2^-40, NaN where counted is 0."""
    q = np.ascontiguousarray(q, dtype=np.int64)
    counted = np.ascontiguousarray(counted, dtype=np.uint32)
    if q.shape != counted.shape or q.ndim != 1:
        raise ValueError("q and counted are one-dimensional and of one length")
    K = q.size
    out = np.full(max(K, 1), 12345.678, dtype=np.float64)
    _abi.check(_abi.load().fmh_ld_score_values(_ptr(q) if K else None, _ptr(counted) if K else None, K, _ptr(out) if K else None))
    return out[:K]


def ldsc_regress(chi2, score, n_samples, m_sites, blocks=200, intercept=None, weights=None) -> dict:
    """fmh_ldsc_regress (host only): the LD score regression of chi2 on score; a dict of LDSC_OUT."""
    chi2 = np.ascontiguousarray(chi2, dtype=np.float64)
    score = np.ascontiguousarray(score, dtype=np.float64)
    if chi2.shape != score.shape or chi2.ndim != 1:
        raise ValueError("chi2 and score are one-dimensional and of one length")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != score.shape:
            raise ValueError("weights has one entry per site")
    out = _abi.LdscOut()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    fixed = None if intercept is None else C.byref(C.c_double(float(intercept)))
    K = chi2.size
    _abi.check(_abi.load().fmh_ldsc_regress(_ptr(chi2) if K else None, _ptr(score) if K else None, _ptr(weights), K, float(n_samples), float(m_sites), int(blocks),
                                            fixed, C.byref(out)))
    return {name: getattr(out, name) for name in LDSC_OUT}


# ---- haplotype homozygosity windows --------------------------------------------------------------------------------------------------
HAP_WINDOW_DTYPE = np.dtype([("sum_sq", np.uint64), ("distinct", np.uint32), ("top", np.uint32, (3,))])
HAP_STATS = ("h1", "h12", "h123", "h2_h1", "haplotype_diversity")
HAP_THREADS = (64, 256, 512, 1024)   # the values FMH_HAP_THREADS takes


@dataclass
class HapWindowsResult:
    sum_sq: np.ndarray           # [n_windows] uint64
    distinct: np.ndarray         # [n_windows] uint32
    top: np.ndarray              # [n_windows][3] uint32
    first: Optional[np.ndarray]  # [n_windows][n] uint32, or None when the partition was not asked for


def haplotype_max_members() -> int:
    """fmh_haplotype_max_members: the largest group fmh_haplotype_windows takes (needs no device)."""
    return int(_abi.load().fmh_haplotype_max_members())


def haplotype_windows(m: DeviceMatrix, g: Groups, windows=None, partition: bool = False, stream=None, fill: Optional[int] = None) -> HapWindowsResult:
    """fmh_haplotype_windows: the identical-haplotype classes of the one group of `g` over row windows [(begin, end), ...] (default: one
    window, every row).  `fill` pre-fills the outputs with that byte (tests: the call must write every entry)."""
    w = np.array([[0, m.variants]] if windows is None else windows, dtype=np.uint64).reshape(-1, 2)
    n_windows, n = w.shape[0], g.sizes[0]
    junk = None if fill is None else np.full(max(HAP_WINDOW_DTYPE.itemsize * n_windows, 4 * n_windows * n, 8), fill, dtype=np.uint8)
    out_bytes = max(HAP_WINDOW_DTYPE.itemsize * n_windows, 8)
    d_out = DeviceBuffer(m.device, out_bytes) if junk is None else DeviceBuffer.from_numpy(m.device, junk[:out_bytes])
    d_first = None
    if partition:
        first_bytes = max(4 * n_windows * n, 8)
        d_first = DeviceBuffer(m.device, first_bytes) if junk is None else DeviceBuffer.from_numpy(m.device, junk[:first_bytes])
    _abi.check(_abi.load().fmh_haplotype_windows(m._h, g._h, _ptr(w), n_windows, d_out.ptr, None if d_first is None else d_first.ptr, stream))
    rec = d_out.to_numpy(np.uint8, HAP_WINDOW_DTYPE.itemsize * n_windows).view(HAP_WINDOW_DTYPE)
    first = None if d_first is None else d_first.to_numpy(np.uint32, n_windows * n).reshape(n_windows, n)
    return HapWindowsResult(rec["sum_sq"].copy(), rec["distinct"].copy(), rec["top"].copy(), first)


def haplotype_stats(sum_sq, distinct, top, n: int) -> Dict[str, np.ndarray]:
    """fmh_haplotype_stats (host only): h1, h12, h123, h2_h1 and haplotype_diversity of window records of a group of n members."""
    sum_sq = np.ascontiguousarray(sum_sq, dtype=np.uint64).reshape(-1)
    rec = np.zeros(sum_sq.size, dtype=HAP_WINDOW_DTYPE)
    rec["sum_sq"], rec["distinct"], rec["top"] = sum_sq, np.asarray(distinct).reshape(-1), np.asarray(top).reshape(-1, 3)
    out = np.zeros((sum_sq.size, len(HAP_STATS)), dtype=np.float64)
    _abi.check(_abi.load().fmh_haplotype_stats(_ptr(rec), sum_sq.size, int(n), _ptr(out)))
    return {name: out[:, i].copy() for i, name in enumerate(HAP_STATS)}


# ---- extended haplotype homozygosity scans -------------------------------------------------------------------------------------------
EHH_SIDE_DTYPE = np.dtype([("area2", np.uint64, (2,)), ("pair_steps", np.uint64, (2,)), ("steps", np.uint32, (2,)), ("core", np.uint32, (2,)),
                           ("flags", np.uint32), ("reserved", np.uint32)])
EHH_STATS = ("ihh", "sl", "ihs", "nsl")
EHH_EDGE0, EHH_EDGE1, EHH_GAP0, EHH_GAP1, EHH_SKIPPED = 1, 2, 4, 8, 16   # fmh_ehh_side.flags


@dataclass
class EhhScanResult:
    sides: np.ndarray            # [n_focal][2] of EHH_SIDE_DTYPE, the left side first
    pairs: Optional[np.ndarray]  # [n_focal][2 sides][2 cores][max_extent] uint32, or None when the curve was not asked for


def ehh_max_members() -> int:
    """fmh_ehh_max_members: the largest group fmh_ehh_scan takes (needs no device)."""
    return int(_abi.load().fmh_ehh_max_members())


def ehh_scan(m: DeviceMatrix, g: Groups, focal, row_begin: int = 0, row_end: Optional[int] = None, positions=None, min_ehh=(0, 1),
             max_extent: int = 0, max_gap: int = 0, min_core: int = 0, curve: bool = False, stream=None, fill: Optional[int] = None) -> EhhScanResult:
    """fmh_ehh_scan: per focal row and side the integer record of the extended haplotype homozygosity scan of the one group of `g` inside
    rows [row_begin, row_end) (default: every row).  `positions` [variants] uint32 or None (x(r) = r); min_ehh = (num, den).  `fill`
    pre-fills the outputs with that byte (tests: the call must write every entry)."""
    row_end = m.variants if row_end is None else row_end
    f = np.ascontiguousarray(focal, dtype=np.uint64).reshape(-1)
    pos = None if positions is None else np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
    if pos is not None and pos.size != m.variants:
        raise ValueError("positions must hold one entry per variant of the matrix")
    params = _abi.EhhParams(int(min_ehh[0]), int(min_ehh[1]), int(max_extent), int(max_gap), int(min_core), 0)
    out_bytes = max(EHH_SIDE_DTYPE.itemsize * 2 * f.size, 8)
    pair_count = 4 * f.size * int(max_extent)
    pair_bytes = max(4 * pair_count, 8)

    def buffer(nbytes):
        return DeviceBuffer(m.device, nbytes) if fill is None else DeviceBuffer.from_numpy(m.device, np.full(nbytes, fill, dtype=np.uint8))

    d_out = buffer(out_bytes)
    d_pairs = buffer(pair_bytes) if curve else None
    _abi.check(_abi.load().fmh_ehh_scan(m._h, g._h, int(row_begin), int(row_end), _ptr(f), f.size, None if pos is None else _ptr(pos), C.byref(params),
                                        d_out.ptr, None if d_pairs is None else d_pairs.ptr, stream))
    sides = d_out.to_numpy(np.uint8, EHH_SIDE_DTYPE.itemsize * 2 * f.size).view(EHH_SIDE_DTYPE).reshape(f.size, 2).copy()
    pairs = None if d_pairs is None else d_pairs.to_numpy(np.uint32, pair_count).reshape(f.size, 2, 2, int(max_extent))
    return EhhScanResult(sides, pairs)


def ehh_stats(sides, include_edges: bool = False) -> Dict[str, np.ndarray]:
    """fmh_ehh_stats (host only): ihh [F][2], sl [F][2], ihs [F] and nsl [F] of records [F][2] of EHH_SIDE_DTYPE."""
    sides = np.ascontiguousarray(sides, dtype=EHH_SIDE_DTYPE).reshape(-1, 2)
    out = np.zeros((sides.shape[0], 6), dtype=np.float64)
    _abi.check(_abi.load().fmh_ehh_stats(_ptr(sides), sides.shape[0], int(bool(include_edges)), _ptr(out)))
    return dict(ihh=out[:, 0:2].copy(), sl=out[:, 2:4].copy(), ihs=out[:, 4].copy(), nsl=out[:, 5].copy())
