"""LD scores and LD score regression where no device is needed: the oracle (tests/ldscore_ref.py) against an independent route (numpy.corrcoef
per pair, math.fsum of the terms), the host-only entry points fmh_ld_scores_host, fmh_ld_score_values and fmh_ldsc_regress against the oracle
(integers with array_equal, doubles bit for bit), the exact 2^40 of a row with itself, its duplicate and its complement, the monomorphic
rows, the refusals in the header's order, the Python argument errors, the empty answers and LdScores.from_q, the regression against
numpy.linalg.lstsq and on a planted model, and the twin run stand-alone under ASan and UBSan (ferromic_amd/csrc/ldscore_host_check.cpp),
whose output is compared with the oracle's over the splitmix64 cohort of tests/clump_ref.py."""

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import clump_ref as R
from tests import ldscore_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.path.join(ROOT, "ferromic_amd", "bin")
ONE = 1 << 40
# fmh_ldsc_regress against numpy.linalg.lstsq on the sqrt(w)-scaled design: the largest relative difference measured over SETS below was
# 9.77e-15 (printed by test_regression_against_lstsq); the bound is 100 x that, test_assoc_cpu.py's margin.
LSTSQ_MEASURED = 9.77e-15
LSTSQ_BOUND = 100 * LSTSQ_MEASURED


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    from ferromic_amd import device

    return device


@pytest.fixture(scope="module")
def fm(dev):
    import ferromic

    return ferromic


def check_twin(dev, d, x, window, adjust, what):
    ref = L.ld_scores(d, x, window, adjust)
    got = dev.ld_scores_host(d, dev.ldscore_params(window, adjust), x=x)
    assert got.q.dtype == np.int64 and np.array_equal(got.q, ref["q"]), what
    assert np.array_equal(got.partners, ref["partners"]) and np.array_equal(got.counted, ref["counted"]), what
    assert R.same_bits(dev.ld_score_values(got.q, got.counted), ref["scores"]), what
    assert dev.ld_scores_host(d, dev.ldscore_params(window, adjust), x=x, want_partners=False).partners is None
    return ref


def test_oracle_counts_are_the_clumping_oracles():
    d = R.mosaic_dosages(40, 23, 3, miss=0.1)
    table = L.pair_table(d)
    for i in range(0, 40, 3):
        for j in range(40):
            assert tuple(int(v) for v in table[i, j]) == R.counts(d[i], d[j]), (i, j)
    x = R.mosaic_positions(40, 3)
    fast, slow = L.ld_scores(d, x, 9, True), L.ld_scores(d, x, 9, True, counts_of=R.counts)
    for name in ("q", "partners", "counted"):
        assert np.array_equal(fast[name], slow[name]), name


@pytest.mark.parametrize("adjust", [False, True])
def test_oracle_against_corrcoef(adjust):
    """The scores differ from an independent route by at most partners * 2^-41 (quantisation) + 8 * 2^-53 * sum |t| (the reference pairs' rounding)."""
    d, x = R.mosaic_dosages(60, 41, 7), R.mosaic_positions(60, 7)
    ref = L.ld_scores(d, x, 30, adjust)
    checked, worst = 0, 0.0
    for i in range(60):
        terms = []
        for j in range(60):
            if abs(int(x[j]) - int(x[i])) > 30:
                continue
            both = (d[i] < 3) & (d[j] < 3)
            ga, gb = d[i][both].astype(float), d[j][both].astype(float)
            if both.sum() == 0 or ga.std() == 0 or gb.std() == 0 or (adjust and both.sum() < 3):
                continue
            r2 = float(np.corrcoef(ga, gb)[0, 1]) ** 2
            terms.append(r2 - (1.0 - r2) / float(both.sum() - 2) if adjust else r2)
        assert len(terms) == ref["counted"][i], i
        if not terms:
            assert math.isnan(ref["scores"][i])
            continue
        bound = int(ref["partners"][i]) * 2.0 ** -41 + 8 * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
        diff = abs(ref["scores"][i] - math.fsum(terms))
        worst = max(worst, diff / bound)
        assert diff <= bound, (i, diff, bound)
        checked += 1
    print("largest difference / bound: %.3g over %d rows (adjust %s)" % (worst, checked, adjust))
    assert checked >= 55


@pytest.mark.parametrize("seed", [1, 2])
def test_twin_against_the_oracle(dev, seed):
    d, x = R.mosaic_dosages(300, 37, seed), R.mosaic_positions(300, seed)
    ref = check_twin(dev, d, x, 90, True, ("mosaic", seed))
    assert (ref["scores"] >= 3).sum() >= 100 and (ref["counted"] == 0).sum() >= 2 and ref["negative_terms"] >= 1000 and (ref["counted"] < ref["partners"]).any()
    check_twin(dev, d, x, 90, False, ("no correction", seed))
    check_twin(dev, d, None, 7, True, ("rows as positions", seed))
    check_twin(dev, d[:120], x[:120], 2**32 - 1, True, ("every site in every window", seed))
    check_twin(dev, d, x, 0, False, ("window 0 with repeated positions", seed))
    check_twin(dev, d[:, :2], x, 90, True, ("two samples: n < 3 everywhere", seed))
    empty = check_twin(dev, d[:0], x[:0], 90, True, "no row")
    assert empty["q"].shape == (0,)


@pytest.mark.parametrize("adjust", [False, True])
def test_exact_terms(dev, adjust):
    d = R.mosaic_dosages(40, 25, 5, miss=0.1)
    # window 0 on distinct positions: a polymorphic row scores itself, exactly 1
    ref = check_twin(dev, d, None, 0, adjust, "window 0")
    poly = np.array([not math.isnan(R.r2_of(R.counts(d[k], d[k]))) for k in range(40)])
    assert poly.sum() >= 30 and not poly[38] and not poly[39]
    assert (ref["q"][poly] == ONE).all() and (ref["counted"][poly] == 1).all() and (ref["partners"] == 1).all()
    # the monomorphic rows: no term of their own (a NaN score) and none in anybody's sum
    assert (ref["counted"][~poly] == 0).all() and (ref["q"][~poly] == 0).all() and np.isnan(ref["scores"][~poly]).all()
    wide = check_twin(dev, d, None, 100, adjust, "everything")
    assert (wide["counted"][~poly] == 0).all() and np.isnan(wide["scores"][~poly]).all() and (wide["partners"] == 40).all()
    without = check_twin(dev, d[:38], None, 100, adjust, "without the monomorphic rows")
    assert np.array_equal(without["q"], wide["q"][:38]) and np.array_equal(without["counted"], wide["counted"][:38])
    # the duplicate (row 1) and the complement (row 2) of row 0 contribute exactly 2^40 to each other
    for other in (1, 2):
        pair = check_twin(dev, d[[0, other]], None, 5, adjust, ("pair", other))
        assert pair["q"].tolist() == [2 * ONE, 2 * ONE] and pair["counted"].tolist() == [2, 2] and pair["scores"].tolist() == [2.0, 2.0]


def test_host_refusals_in_order(dev):
    lib, abi = dev._abi.load(), dev._abi
    d = np.zeros((3, 2), dtype=np.uint8)
    x = np.array([5, 4, 6], dtype=np.uint32)
    q, counted = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    ok, bad = dev.ldscore_params(5), dev.ldscore_params(5)
    bad.flags = 6

    def status(call):
        s = call()
        return s, lib.fmh_last_error().decode()

    host = lib.fmh_ld_scores_host
    assert status(lambda: host(ptr(d), None, 3, 2, None, None, None, None)) == (abi.FMH_ERR_INVALID, "NULL params")
    assert status(lambda: host(ptr(d), None, 3, 0, C.byref(bad), None, None, None)) == (abi.FMH_ERR_INVALID, "NULL h_q")
    assert status(lambda: host(ptr(d), None, 3, 0, C.byref(bad), ptr(q), None, None)) == (abi.FMH_ERR_INVALID, "NULL h_counted")
    assert status(lambda: host(None, None, 3, 0, C.byref(bad), ptr(q), None, ptr(counted))) == (abi.FMH_ERR_INVALID, "n_samples is 0")
    assert status(lambda: host(None, None, 3, 2, C.byref(bad), ptr(q), None, ptr(counted))) == (abi.FMH_ERR_INVALID, "NULL dosage")
    four = np.array([[0, 1], [4, 1], [0, 0]], dtype=np.uint8)
    assert status(lambda: host(ptr(four), ptr(x), 3, 2, C.byref(bad), ptr(q), None, ptr(counted)))[1] == "dosage 4 (row 1, sample 0) is not 0, 1, 2 or 3"
    assert status(lambda: host(ptr(d), ptr(x), 3, 2, C.byref(bad), ptr(q), None, ptr(counted))) == (abi.FMH_ERR_INVALID, "flags other than 0 or FMH_LDSCORE_ADJUST (flags 6)")
    assert status(lambda: host(ptr(d), ptr(x), 3, 2, C.byref(ok), ptr(q), None, ptr(counted))) == (abi.FMH_ERR_INVALID, "the positions descend at row 1")
    assert host(None, None, 0, 2, C.byref(ok), None, None, None) == abi.FMH_OK
    # the device call: what is refused before a matrix is looked at
    assert status(lambda: lib.fmh_ld_scores(None, None, 2, 0, 3, None, None, None, None, None, None, None)) == (abi.FMH_ERR_INVALID, "NULL matrix")
    # the values and the regression
    assert status(lambda: lib.fmh_ld_score_values(None, None, 2, None)) == (abi.FMH_ERR_INVALID, "a NULL sum, count or output with 2 rows")
    assert lib.fmh_ld_score_values(None, None, 0, None) == abi.FMH_OK
    y, l = np.full(12, 1.5), np.arange(12) + 1.0
    out = abi.LdscOut()

    def regress(chi2=y, score=l, K=12, N=10.0, M=12.0, blocks=3, fixed=None, o=out):
        return lib.fmh_ldsc_regress(None if chi2 is None else ptr(chi2), ptr(score), None, K, N, M, blocks, fixed, None if o is None else C.byref(o))

    neg = y.copy()
    neg[3] = -1.0
    nan = C.byref(C.c_double(math.nan))
    for make, words in [(lambda: regress(o=None, chi2=None), "NULL out"), (lambda: regress(chi2=None, N=0.0), "NULL chi2 or score with 12 sites"),
                        (lambda: regress(N=0.0, M=math.inf), "N and M must be finite and above 0"), (lambda: regress(M=math.nan, fixed=nan), "N and M must be finite and above 0"),
                        (lambda: regress(fixed=nan, blocks=1), "the fixed intercept is not finite"), (lambda: regress(blocks=1, chi2=neg), "at least 2 blocks are required"),
                        (lambda: regress(blocks=4, chi2=neg), "fewer than 2 used sites per fitted parameter and block"), (lambda: regress(chi2=neg), "a chi2 is negative")]:
        s, message = status(make)
        assert s == abi.FMH_ERR_INVALID and message.startswith(words), (message, words)
    assert regress() == abi.FMH_OK and out.n_used == 12 and out.blocks == 3
    assert regress(blocks=6, fixed=C.byref(C.c_double(1.0))) == abi.FMH_OK and out.blocks == 6 and math.isnan(out.intercept_se)   # one parameter: 2 sites per block do


# ---- the regression ------------------------------------------------------------------------------------------------------------------------------
def regression_set(seed, K, nan_share=0.02):
    rng = np.random.default_rng(seed)
    score = np.abs(rng.gamma(2.0, 20.0, size=K)) + rng.integers(0, 2, size=K) * 0.25
    N, M = float(rng.integers(500, 50_000)), float(K)
    chi2 = rng.chisquare(1, size=K) * (1.05 + 0.3 * N * score / M)
    weights = score * rng.uniform(0.5, 1.5, size=K)
    chi2[rng.random(K) < nan_share] = np.nan
    score[rng.random(K) < nan_share] = np.nan
    return chi2, score, weights, N, M


SETS = [(1, 400, 20, None, False), (2, 1000, 200, None, True), (3, 57, 7, None, False), (4, 800, 50, 1.0, True), (5, 300, 2, 1.2, False)]


@pytest.mark.parametrize("seed,K,blocks,intercept,weighted", SETS)
def test_regression_against_the_oracle(dev, seed, K, blocks, intercept, weighted):
    chi2, score, weights, N, M = regression_set(seed, K)
    w = weights if weighted else None
    ref = L.regress(chi2, score, N, M, blocks, intercept, w)
    got = dev.ldsc_regress(chi2, score, N, M, blocks, intercept, w)
    for name in dev.LDSC_OUT[:7]:
        assert R.same_bits([got[name]], [ref[name]]), (name, got[name], ref[name])
    assert got["n_used"] == ref["n_used"] < K and got["blocks"] == ref["blocks"] == blocks
    assert ref["h2_se"] > 0 and (intercept is None) == (not math.isnan(ref["intercept_se"]))


def test_regression_against_lstsq(dev):
    worst = 0.0
    for seed, K, blocks, intercept, weighted in SETS:
        chi2, score, weights, N, M = regression_set(seed, K)
        ref = L.regress(chi2, score, N, M, blocks, intercept, weights if weighted else None)
        got = dev.ldsc_regress(chi2, score, N, M, blocks, intercept, weights if weighted else None)
        root = np.sqrt(np.array(ref["w"]))
        x, y = np.array(ref["x"]), np.array(ref["y"])
        if intercept is None:
            (a, h), *_ = np.linalg.lstsq(np.stack([root, root * x], axis=1), root * y, rcond=None)
            worst = max(worst, abs(got["intercept"] - a) / abs(a))
        else:
            (h,), *_ = np.linalg.lstsq((root * x)[:, None], root * (y - intercept), rcond=None)
        worst = max(worst, abs(got["h2"] - h) / abs(h))
    print("largest relative difference from lstsq: %.3g" % worst)
    assert worst <= LSTSQ_BOUND, worst


def test_planted_model_is_recovered(dev):
    rng = np.random.default_rng(11)
    K, N, M = 2000, 2_000.0, 2000.0
    score = rng.gamma(3.0, 15.0, size=K) + 1.0
    x = N * score / M
    chi2 = 1.1 + 0.4 * x + rng.normal(0.0, 1.0, size=K) * 0.2 * (1.1 + 0.4 * x)
    chi2 = np.maximum(chi2, 0.0)
    ref = L.regress(chi2, score, N, M)
    assert ref["blocks"] == 200 and ref["n_used"] == K
    assert abs(ref["h2"] - 0.4) <= 3 * ref["h2_se"] and abs(ref["intercept"] - 1.1) <= 3 * ref["intercept_se"], ref   # on the oracle first
    assert 0 < ref["h2_se"] < 0.05 and 0 < ref["intercept_se"] < 0.5
    got = dev.ldsc_regress(chi2, score, N, M)
    assert abs(got["h2"] - 0.4) <= 3 * got["h2_se"] and abs(got["intercept"] - 1.1) <= 3 * got["intercept_se"]
    assert R.same_bits([got[k] for k in dev.LDSC_OUT[:7]], [ref[k] for k in dev.LDSC_OUT[:7]])
    fixed = dev.ldsc_regress(chi2, score, N, M, intercept=1.1)
    assert fixed["intercept"] == 1.1 and abs(fixed["h2"] - 0.4) <= 3 * fixed["h2_se"] and fixed["h2_se"] < got["h2_se"]


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------
def records(n_sites=5, n_samples=3):
    return [dict(position=10 * i, genotypes=[[(i + s) & 1, (i * s) & 1] for s in range(n_samples)]) for i in range(n_sites)]


def refused(message, call, kind=ValueError):
    with pytest.raises(kind) as caught:
        call()
    assert str(caught.value) == message, (str(caught.value), message)


def empty(s, rows, window=1_000_000, adjusted=True, n_samples=3):
    assert len(s) == rows and s.m_sites == 0
    assert repr(s) == "LdScores(rows=%d, scored=0, window=%d, adjusted=%s, n_samples=%d)" % (rows, window, adjusted, n_samples)
    assert s.q.dtype == np.int64 and s.q.tolist() == [0] * rows
    assert s.partners.dtype == np.uint32 and s.partners.tolist() == [0] * rows and s.counted.dtype == np.uint32 and s.counted.tolist() == [0] * rows
    assert s.scores.dtype == np.float64 and s.scores.shape == (rows,) and np.isnan(s.scores).all()
    assert s.window == window and s.adjusted is adjusted and s.n_samples == n_samples


def test_python_surface_without_a_device(fm):
    V = records()
    assert fm.LdScores.__module__.endswith("_core") and callable(fm.ld_scores) and callable(fm.ld_score_regression) and hasattr(fm.Population, "ld_scores")
    none = fm.ld_scores(V, sites=np.zeros(5, dtype=bool))                           # no kept row
    empty(none, 5)
    assert none.positions.tolist() == [0, 10, 20, 30, 40]
    empty(fm.ld_scores(V, window=7, adjust=False, region=(1000, 2000)), 0, window=7, adjusted=False)
    pop = fm.Population.from_numpy("p", np.zeros((4, 3, 2), dtype=np.int8), np.arange(4) * 10, [(0, 0), (0, 1), (2, 0)], 100)
    empty(pop.ld_scores(sites=np.zeros(4, dtype=bool)), 4, n_samples=1)
    # argument errors, the window first
    refused("window must be within 0 .. 2^32 - 1", lambda: fm.ld_scores(V, window=-1, samples=[7]))
    refused("window must be within 0 .. 2^32 - 1", lambda: fm.ld_scores(V, window=2**32))
    refused("sample 7 is outside the variants' 3 samples", lambda: fm.ld_scores(V, samples=[7], sites=np.ones(4, dtype=bool)))
    refused("at least one sample is required for LD scores", lambda: fm.ld_scores(V, samples=[], sites=np.ones(4, dtype=bool)))
    refused("sites has 4 entries for 5 rows", lambda: fm.ld_scores(V, sites=np.ones(4, dtype=bool)))
    down = [dict(position=q, genotypes=[[0, 0], [0, 0]]) for q in (10, 30, 20)]
    refused("the positions descend at variant 2: the LD scores need them in order", lambda: fm.ld_scores(down))
    haploid = [dict(position=1, genotypes=[[0], [1]])]
    refused("the LD scores take diploid genotypes (ploidy 2), got ploidy 1", lambda: fm.ld_scores(haploid))
    # from_q: the scores of given sums, no device
    s = fm.LdScores.from_q([3 * ONE + (ONE >> 1), 0, -ONE], [4, 0, 2], partners=[5, 2, 2], positions=[7, 8, 9], window=50, adjusted=False, n_samples=12)
    assert R.same_bits(s.scores, [3.5, math.nan, -1.0]) and s.m_sites == 2 and len(s) == 3 and s.partners.tolist() == [5, 2, 2]
    assert repr(s) == "LdScores(rows=3, scored=2, window=50, adjusted=False, n_samples=12)" and s.positions.tolist() == [7, 8, 9]
    assert fm.LdScores.from_q([ONE], [1]).partners.tolist() == [1] and fm.LdScores.from_q([], []).scores.shape == (0,)
    refused("counted has 1 entries, expected 2", lambda: fm.LdScores.from_q([0, 0], [1]))
    refused("counted exceeds partners at row 1", lambda: fm.LdScores.from_q([0, 0], [1, 3], partners=[1, 2]))
    # the regression through both doors, against the oracle
    chi2, score, weights, N, M = regression_set(2, 1000)
    counted = np.where(np.isnan(score), 0, 3).astype(np.uint32)
    q = np.where(np.isnan(score), 0, np.rint(np.nan_to_num(score) * ONE)).astype(np.int64)
    s = fm.LdScores.from_q(q, counted, n_samples=int(N))
    exact = L.values(q, counted)
    assert R.same_bits(s.scores, exact)
    for kw in (dict(), dict(blocks=20, intercept=1.0), dict(weights=weights, m_sites=5000)):
        ref = L.regress(chi2, exact, N, kw.get("m_sites", int(np.isfinite(exact).sum())), kw.get("blocks", 200), kw.get("intercept"), kw.get("weights"))
        for got in (s.regression(chi2, **kw), fm.ld_score_regression(chi2, exact, N, **kw)):
            assert isinstance(got, fm.LdScoreRegression) and repr(got).startswith("LdScoreRegression(h2=")
            for name in ("h2", "h2_se", "intercept", "intercept_se", "ratio", "mean_chi2", "lambda_gc"):
                assert R.same_bits([getattr(got, name)], [ref[name]]), (name, kw)
            assert got.n_used == ref["n_used"] and got.blocks == ref["blocks"] and got.fixed_intercept == kw.get("intercept")
    refused("chi2 has 3 entries for 1000 sites", lambda: s.regression(np.ones(3)))
    refused("weights has 3 entries for 1000 sites", lambda: s.regression(chi2, weights=np.ones(3)))
    refused("chi2 must be a one-dimensional float array", lambda: fm.ld_score_regression(np.ones((2, 2)), np.ones(4), 10))
    refused("n_samples must be a number", lambda: fm.ld_score_regression(chi2, exact, "many"))
    refused("m_sites must be a number", lambda: s.regression(chi2, m_sites="all"))
    refused("intercept must be a number", lambda: s.regression(chi2, intercept=[1.0]))
    with pytest.raises(ValueError, match="at least 2 blocks are required"):
        s.regression(chi2, blocks=1)
    with pytest.raises(ValueError, match="N and M must be finite and above 0"):
        fm.ld_score_regression(chi2, exact, 0)


def test_twin_under_sanitizers(dev):
    program = os.path.join(BIN_DIR, "ldscore_host_check.asan")
    res = subprocess.run(["make", "-C", os.path.join(ROOT, "ferromic_amd", "csrc"), program], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    terms_total = regressions = 0
    for seed, K, n, window, flags in ((5, 300, 37, 60, 1), (9, 129, 17, 3, 0), (2, 64, 1, 0, 1), (3, 1, 5, 0, 0), (4, 70, 2, 2**32 - 1, 1)):
        d, x, _ = R.splitmix_cohort(seed, K, n)
        ref = L.ld_scores(d, x, window, bool(flags))
        terms, h = L.checksum(ref)
        terms_total += terms
        rnd = R.SplitMix64(seed + 1)
        chi2 = [float(rnd() % 4096) / 1024.0 for _ in range(K)]
        try:
            fit = L.regress(chi2, ref["scores"], float(n), float(K), 4)
            second = "ldscore_host_check: regression %016x %016x %016x %016x used %d\n" % tuple([L.bits_of(fit[k]) for k in ("h2", "h2_se", "intercept", "intercept_se")] + [fit["n_used"]])
            regressions += 1
        except ValueError:
            second = "ldscore_host_check: regression refused: fewer than 2 used sites per fitted parameter and block\n"
        res = subprocess.run([program] + [str(a) for a in (seed, K, n, window, flags)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        want = "ldscore_host_check: %d rows x %d samples, %d terms, checksum %016x\n" % (K, n, terms, h) + second
        assert res.stdout == want, (res.stdout, want)
    assert terms_total > 20_000 and regressions >= 2
    # the partner ranges and the 2^22 rule (fmh_ld_scores' refusal), on repeated positions: rows k at positions k // every
    limit = 1 << 22
    for K, window, every, refused_row in ((limit + 5, 0, limit + 5, 0), (limit + 5, 0, limit, -1), (limit + 5, 1, limit // 2, limit // 2), (3 * limit // 2 + 3, limit // 2, 1, limit // 2),
                                          (3 * limit // 2 + 3, limit // 2 - 1, 1, -1), (1000, 7, 3, -1)):
        pos = np.arange(K, dtype=np.int64) // every
        partners = np.searchsorted(pos, pos + window, side="right") - np.searchsorted(pos, pos - window, side="left")
        over = np.flatnonzero(partners > limit)
        assert (int(over[0]) if over.size else -1) == refused_row, (K, window, every)
        res = subprocess.run([program, "ranges", str(K), str(window), str(every)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        want = "ldscore_host_check: ranges of %d rows, window %d: %d partners in all, at most %d, first refused row %d\n" % (K, window, int(partners.sum()), int(partners.max()),
                                                                                                                         refused_row)
        assert res.stdout == want, (res.stdout, want)
