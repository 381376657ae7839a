"""The polygenic score without a GPU: the library's host functions (fmh_score_exponents, fmh_score_values, fmh_score_stats,
ferromic.PolygenicScore.from_sums) against tests/score_ref.py - integers with array_equal, doubles bitwise -, the three modes of the
DEFINITION against a float dot product of the mean-imputed, centred or zero-filled dosage, every refusal that needs no device, and the Python
argument errors.

The bound against the float dot product is derived, not chosen.  In units of 2^-e_k a used row contributes c g V + (1 - c) U (mean),
c (g V - U) (center) or c g V (zero) with V and U each rounded once, by at most 0.5: at most g * 0.5 + 0.5 <= 1.5 per used row, so
|score - exact| <= rows_used * 1.5 * 2^-e_k; the f64 dot product it is compared with is itself off by at most rows * 2^-53 * sum |terms|.
Measured by this file's seeded set: at most 0.09 of the bound (printed by the test)."""

import ctypes as C

import numpy as np
import pytest

from tests import score_ref as R


@pytest.fixture(scope="module")
def dev():
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def lib():
    from ferromic_amd import _abi

    return _abi.load()


def cohort(rows, n, seed, missing=True):
    """(alleles [rows][2 n] uint8 with some alleles 2, called [rows][2 n] bool); row 3 is uncalled everywhere, row 5 has no alt allele."""
    rng = np.random.default_rng(seed)
    freq = rng.beta(0.5, 1.2, size=rows)
    x = (rng.random((rows, 2 * n)) < freq[:, None]).astype(np.uint8)
    x[(rng.random((rows, 2 * n)) < 0.01)] = 2
    called = rng.random((rows, 2 * n)) >= (0.08 if missing else 0.0)
    if rows > 5:
        called[3] = False
        x[5] = 0
    return x, called


def weights_for(rows, K, seed):
    """Columns of very different scales; row 7 is all zero; column 2 (when there) is zero everywhere."""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(rows, K)) * np.array([10.0 ** ((5 * k) % 23 - 11) for k in range(K)])
    if rows > 7:
        w[7] = 0.0
    if K > 2:
        w[:, 2] = 0.0
    return w


def test_symbols_are_exported_and_prototyped(lib):
    from ferromic_amd import _abi

    header = open(_abi.LIB_PATH.replace("ferromic_amd/lib/libferromic_hip.so", "include/ferromic_hip.h")).read()
    for name in ("fmh_score_sums", "fmh_score_exponents", "fmh_score_values", "fmh_score_stats"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS and ("int " + name + "(") in header, name
    assert len(_abi.SYMBOLS["fmh_score_sums"][1]) == 11
    for key, default in (("FMH_SCORE_ITEM_ROWS", 0), ("FMH_SCORE_BUDGET_BYTES", 1 << 30)):
        assert _abi.get_option(key) == default


# ---- exponents, values, stats against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(1, 1), (40, 3), (200, 16), (64, 64)])
def test_host_functions_match_oracle(dev, rows, K):
    n = 30
    x, called = cohort(rows, n, seed=rows + K)
    w = weights_for(rows, K, seed=7 * rows + K)
    e = R.exponents(w)
    got_e = dev.score_exponents(w)
    assert got_e.dtype == np.int32 and got_e.tolist() == e
    trk = R.tracks(x, called)
    ref = R.values(w, e, *trk)
    got = dev.score_values(w, got_e, *trk)
    assert got.dosage.dtype == np.int32 and np.array_equal(got.dosage, ref["V"]) and np.array_equal(got.called, ref["U"])
    assert got.called_total.tolist() == ref["total"] and np.array_equal(got.row_used, ref["used"])
    nonzero = [k for k in range(K) if w[:, k].any()]
    assert np.abs(got.dosage[:, nonzero]).max(axis=0).min() > 1 << 28 and np.abs(got.dosage).max() <= 1 << 29   # every column uses the range
    assert np.abs(got.called).max() <= 1 << 30
    no_tracks = dev.score_values(w, got_e)
    assert no_tracks.called is None and no_tracks.called_total is None and np.array_equal(no_tracks.row_used, w.any(axis=1))
    assert np.array_equal(no_tracks.dosage[no_tracks.row_used], R.values(w, e)["V"][no_tracks.row_used])
    zero_mode = dev.score_values(w, got_e, *trk, called=False)          # tracks for the unused rows, no U
    assert zero_mode.called is None and np.array_equal(zero_mode.dosage, ref["V"]) and np.array_equal(zero_mode.row_used, ref["used"])
    S, Cs = R.sums(x, called, ref["V"], ref["U"])
    if rows >= 40:
        assert (Cs != np.array(ref["total"])).any() and (Cs != S).any()
    for mode in R.MODES:
        want = R.stats(S, Cs, ref["total"], e, mode)
        have = dev.score_stats(S, got_e, None if mode == "zero" else Cs, got.called_total if mode == "mean" else None, mode)
        assert have.dtype == np.float64 and R.same_f64(have, want), mode


def test_exponent_edges(dev):
    tiny = 5e-324                                   # the smallest subnormal: 0.5 * 2^-1073
    w = np.array([[4.0, 0.0, tiny, 3.0, 1e308],
                  [-1.0, 0.0, 0.0, -3.999, -1.7e308]])
    e = dev.score_exponents(w)
    # 2 * 4 * 2^27 = 2^30 exactly; zeros; 2 * 2^-1074 * 2^1103 = 2^30; 2 * 3.999 * 2^27 < 2^30 <= 2 * 3.999 * 2^28; 2 * 1.7e308 overflows an f64
    assert e.tolist() == [27, 0, 1103, 27, 29 - 1024] == R.exponents(w)
    got, ref = dev.score_values(w, e), R.values(w, R.exponents(w))
    assert np.array_equal(got.dosage, ref["V"])
    assert got.dosage[0].tolist()[:3] == [1 << 29, 0, 1 << 29] and got.dosage[1, 0] == -(1 << 27)
    for k in range(5):
        if k != 1:
            m = float(np.abs(w[:, k]).max())
            assert 2.0 * np.ldexp(m, int(e[k])) <= 2.0 ** 30 < 2.0 * np.ldexp(m, int(e[k]) + 1), k
    # the scores of one sample that is hom-alt everywhere: 2 * (w0 + w1) per column, exactly where the weights are exact in fixed point
    S = 2 * got.dosage.astype(np.int64).sum(axis=0, keepdims=True)
    score = dev.score_stats(S, e, mode="zero")
    assert score[0, 0] == 6.0 and score[0, 1] == 0.0 and score[0, 2] == 2 * tiny


def test_rows_without_calls_and_rows_of_zero_weights_are_unused(dev):
    rows, n, K = 12, 9, 3
    x, called = cohort(rows, n, seed=5)
    w = np.random.default_rng(6).normal(size=(rows, K))
    w[7] = 0.0
    w[8, 1:] = 0.0                                  # one nonzero weight keeps the row
    trk = R.tracks(x, called)
    assert trk[0][3] + trk[1][3] + trk[2][3] == 0
    e = dev.score_exponents(w)
    got = dev.score_values(w, e, *trk)
    assert got.row_used.tolist() == [r not in (3, 7) for r in range(rows)]
    assert not got.dosage[[3, 7]].any() and not got.called[[3, 7]].any() and got.dosage[8, 0] != 0 and not got.dosage[8, 1:].any()
    assert got.called_total.tolist() == got.called.astype(np.int64).sum(axis=0).tolist()
    assert np.array_equal(got.called[5], np.zeros(K, dtype=np.int32)), "a row without alt alleles has mu = 0"


def test_modes_against_a_float_dot_product(dev, capsys):
    worst = 0.0
    for rows, n, K, seed in ((300, 40, 4, 1), (1000, 25, 16, 2), (64, 70, 1, 3)):
        x, called = cohort(rows, n, seed=seed)
        w = weights_for(rows, K, seed=seed + 10)
        e = dev.score_exponents(w)
        trk = R.tracks(x, called)
        val = dev.score_values(w, e, *trk)
        S, Cs = R.sums(x, called, val.dosage, val.called)
        c, g = R.genotypes(x, called)
        N = (trk[0].astype(np.float64) + trk[1] + trk[2])
        with np.errstate(invalid="ignore"):
            mu = np.where(N > 0, (trk[1] + 2.0 * trk[2]) / N, 0.0)
        used = val.row_used.astype(np.float64)[:, None]
        dosage = {"mean": np.where(c == 1, g, mu[:, None]) * used, "center": (g - mu[:, None]) * c * used, "zero": g * used}
        for mode in R.MODES:
            got = dev.score_stats(S, e, None if mode == "zero" else Cs, val.called_total if mode == "mean" else None, mode)
            want = dosage[mode].T @ w
            own = rows * 2.0 ** -53 * (np.abs(dosage[mode]).T @ np.abs(w))
            bound = val.row_used.sum() * 1.5 * np.ldexp(1.0, -e.astype(np.int64))[None, :] + own
            ratio = np.abs(got - want) / bound
            assert (ratio <= 1.0).all(), (mode, rows, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    with capsys.disabled():
        print(f"\npolygenic score vs float dot product: worst |error| / bound {worst:.3f}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_no_device(lib):
    from ferromic_amd import _abi

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rows, K = 6, 2
    w = np.arange(1.0, 1.0 + rows * K).reshape(rows, K)
    e, V, U, T, used = np.zeros(K, np.int32), np.zeros((rows, K), np.int32), np.zeros((rows, K), np.int32), np.zeros(K, np.int64), np.zeros(rows, np.uint8)
    trk = [np.full(rows, 3, np.uint32) for _ in range(3)]
    # fmh_score_exponents(weights, rows, K, e)
    assert lib.fmh_score_exponents(ptr(w), rows, K, ptr(e)) == _abi.FMH_OK and e.tolist() == [25, 25]
    for args in ((None, rows, K, ptr(e)), (ptr(w), rows, K, None), (ptr(w), rows, 0, ptr(e)), (ptr(w), 1, 65, ptr(e))):
        assert lib.fmh_score_exponents(*args) == _abi.FMH_ERR_INVALID, args
    assert lib.fmh_score_exponents(None, 0, K, ptr(e)) == _abi.FMH_OK and e.tolist() == [0, 0]
    for bad in (np.nan, np.inf, -np.inf):
        z = w.copy()
        z[4, 1] = bad
        assert lib.fmh_score_exponents(ptr(z), rows, K, ptr(e)) == _abi.FMH_ERR_INVALID and b"not finite" in lib.fmh_last_error()
    assert lib.fmh_score_exponents(ptr(w), rows, K, ptr(e)) == _abi.FMH_OK
    # fmh_score_values(weights, rows, K, e, hom_ref, het, hom_alt, V, U, T, used)
    good = [ptr(w), rows, K, ptr(e), ptr(trk[0]), ptr(trk[1]), ptr(trk[2]), ptr(V), ptr(U), ptr(T), ptr(used)]
    assert lib.fmh_score_values(*good) == _abi.FMH_OK and used.all() and np.array_equal(U, V) and T.tolist() == V.sum(axis=0).tolist()
    for i in (0, 3, 4, 5, 6, 7, 8, 9, 10):            # a NULL weights, e, one track, V, U without T, T without U, used
        args = list(good)
        args[i] = None
        assert lib.fmh_score_values(*args) == _abi.FMH_ERR_INVALID, i
    args = list(good)
    args[4] = args[5] = args[6] = None                 # U without tracks
    assert lib.fmh_score_values(*args) == _abi.FMH_ERR_INVALID
    args[8] = args[9] = None                           # neither: fine
    assert lib.fmh_score_values(*args) == _abi.FMH_OK
    for i, v in ((2, 0), (2, 65)):
        args = list(good)
        args[i] = v
        assert lib.fmh_score_values(*args) == _abi.FMH_ERR_INVALID, (i, v)
    z = w.copy()
    z[2, 0] = np.nan
    assert lib.fmh_score_values(ptr(z), *good[1:]) == _abi.FMH_ERR_INVALID and b"not finite" in lib.fmh_last_error()
    steep = e + 1                                      # an exponent that is not the column's: 2 |w| 2^e > 2^30
    assert lib.fmh_score_values(*(good[:3] + [ptr(steep)] + good[4:])) == _abi.FMH_ERR_INVALID and b"exponent" in lib.fmh_last_error()
    assert lib.fmh_score_values(None, 0, K, ptr(e), None, None, None, None, None, None, None) == _abi.FMH_OK
    # fmh_score_stats(S, C, T, e, n, K, mode, out)
    n = 3
    S, Cs, out = np.ones((n, K), np.int64), np.ones((n, K), np.int64), np.zeros((n, K))
    good = [ptr(S), ptr(Cs), ptr(T), ptr(e), n, K, 0, ptr(out)]
    assert lib.fmh_score_stats(*good) == _abi.FMH_OK
    for i in (0, 1, 2, 3, 7):
        args = list(good)
        args[i] = None
        assert lib.fmh_score_stats(*args) == _abi.FMH_ERR_INVALID, i
    for i, v in ((5, 0), (5, 65), (6, 3), (6, -1)):
        args = list(good)
        args[i] = v
        assert lib.fmh_score_stats(*args) == _abi.FMH_ERR_INVALID, (i, v)
    assert lib.fmh_score_stats(ptr(S), ptr(Cs), None, ptr(e), n, K, 1, ptr(out)) == _abi.FMH_OK       # center needs no totals
    assert lib.fmh_score_stats(ptr(S), None, None, ptr(e), n, K, 2, ptr(out)) == _abi.FMH_OK          # zero needs neither
    assert lib.fmh_score_stats(ptr(S), None, None, ptr(e), n, K, 1, ptr(out)) == _abi.FMH_ERR_INVALID
    assert lib.fmh_score_stats(None, None, None, None, 0, K, 0, None) == _abi.FMH_OK
    # fmh_score_sums: the first refusal needs no matrix
    assert lib.fmh_score_sums(None, None, 1, 0, 0, ptr(V), None, K, None, None, None) == _abi.FMH_ERR_INVALID and b"NULL matrix" in lib.fmh_last_error()


# ---- ferromic.PolygenicScore.from_sums and the argument errors ---------------------------------------------------------------------------
def test_from_sums_round_trip():
    import ferromic as fm

    rows, n, K = 90, 33, 5
    x, called = cohort(rows, n, seed=21)
    w = weights_for(rows, K, seed=22)
    positions = np.arange(rows, dtype=np.int64) * 10 + 3
    for mode, (missing, center) in {"mean": ("mean", False), "center": ("mean", True), "zero": ("zero", False)}.items():
        ref = R.score(x, called, w, mode=mode)
        got = fm.PolygenicScore.from_sums(ref["S"], ref["e"], None if mode == "zero" else ref["C"], ref["total"] if mode == "mean" else None,
                                          missing=missing, center=center, rows_used=ref["rows_used"], n_called=ref["n_called"],
                                          sample_dosage_sum=ref["dosage_sum"], positions=positions)
        assert len(got) == n and got.mode == mode and got.rows_used == ref["rows_used"] == rows - 2
        assert got.score.shape == (n, K) and R.same_f64(got.score, ref["score"]), mode
        assert R.same_f64(got.average, ref["score"] / float(2 * ref["rows_used"])), mode
        assert np.array_equal(got.n_called, ref["n_called"]) and np.array_equal(got.dosage_sum, ref["dosage_sum"])
        assert got.exponents.dtype == np.int32 and got.exponents.tolist() == ref["e"] and np.array_equal(got.positions, positions)
        assert repr(got) == f"PolygenicScore(samples={n}, columns={K}, rows_used={rows - 2}, mode={mode})"
    ref = R.score(x, called, w, mode="mean")
    for bad in (dict(called_sum=None), dict(called_total=None), dict(called_sum=ref["C"][:3]), dict(missing="median"), dict(missing="zero", center=True),
                dict(dosage_sum=ref["S"].reshape(-1)[:-1]), dict(exponents=[]), dict(n_called=ref["n_called"][:3])):
        kw = dict(dosage_sum=ref["S"], exponents=ref["e"], called_sum=ref["C"], called_total=ref["total"])
        kw.update(bad)
        with pytest.raises(ValueError):
            fm.PolygenicScore.from_sums(**kw)


def test_python_argument_errors_come_before_any_device_use():
    """Without a GPU every one of these would otherwise end in a device error: they are ValueErrors raised first."""
    import ferromic as fm

    x, called = cohort(20, 6, seed=31)
    variants = [dict(position=100 + 10 * i, genotypes=[None if not (called[i, 2 * s] and called[i, 2 * s + 1]) else [int(x[i, 2 * s] & 1), int(x[i, 2 * s + 1] & 1)]
                                                      for s in range(6)]) for i in range(20)]
    w = np.random.default_rng(32).normal(size=(20, 3))
    nan = w.copy()
    nan[4, 1] = np.nan
    for weights, kw in ((w[:19], {}), (w.reshape(20, 3, 1), {}), (nan, {}), (np.inf * w, {}), (np.ones((20, 65)), {}), (np.ones((20, 0)), {}),
                        (w, dict(missing="zero", center=True)), (w, dict(missing="drop")), (w, dict(samples=[2, 1])), (w, dict(samples=[6])),
                        (w, dict(samples=[])), (w[:5], dict(region=(95, 300))), ("weights", {})):
        with pytest.raises(ValueError):
            fm.polygenic_score(variants, weights, **kw)
    big = (1 << 21) + 1                                  # one row more than a call's sums stay exact for
    pop = fm.Population.from_numpy("p", np.zeros((big, 1, 2), dtype=np.int8), np.arange(big, dtype=np.int64), [(0, 0), (0, 1)], big)
    with pytest.raises(ValueError, match="split"):
        pop.polygenic_score(np.ones(big))
    for weights, kw in ((np.ones(big - 2), {}), (np.ones((big - 1, 65)), {}), (np.ones(big - 1), dict(missing="zero", center=True))):
        with pytest.raises(ValueError):
            pop.polygenic_score(weights, **kw)
    haploid = [dict(position=100 + i, genotypes=[[int(x[i, s] & 1)] for s in range(6)]) for i in range(20)]
    with pytest.raises(ValueError):
        fm.polygenic_score(haploid, w)
