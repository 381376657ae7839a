"""GPU-free checks of the haplotype PCA: the numpy restatement (tests/pca_ref.py) against independent routes, the site filter's known
answers, the module's validation (which must not need a device), the TSV text and the combiner, and the library's host eigen solver."""

import os

import numpy as np
import pytest

from tests import pca_ref as R


@pytest.fixture(scope="module")
def fm():
    import __graft_entry__ as ge

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "ferromic_amd", "lib", "libferromic_hip.so")):
        ge.build()
    import ferromic

    return ferromic


def cohort(seed=1, variants=400, samples=30):
    return R.pybench_cohort(variants, samples, seed=seed)


# ---- the restatement against independent routes --------------------------------------------------------------------------------
def test_restatement_equals_svd_route():
    g = cohort()
    kept, _ = R.site_filter(g)
    x = R.haplotype_matrix(g, kept)
    a, w = R.transform(x, 5)
    b = R.transform_svd(x, 5)
    assert a.shape == b.shape == (60, 5)
    assert np.abs(R.canonical_signs(a) - R.canonical_signs(b)).max() <= 1e-10
    # eigenvalues of the Gram are the squared singular values over n - 1
    s = np.linalg.svd(R.standardize(x.copy()), compute_uv=False)
    assert np.allclose(w[:5], s[:5] ** 2 / 59.0, rtol=1e-12)


def test_restatement_equals_sklearn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    g = cohort(seed=2)
    kept, _ = R.site_filter(g)
    x = R.haplotype_matrix(g, kept)
    a, _ = R.transform(x, 4)
    b = decomposition.PCA(n_components=4, svd_solver="full").fit_transform(R.standardize(x.copy()))
    assert np.abs(R.canonical_signs(a) - R.canonical_signs(b)).max() <= 1e-10


def test_features_not_above_haplotypes_give_min_columns():
    g = cohort(seed=3, variants=400, samples=6)
    kept, _ = R.site_filter(g)
    x = R.haplotype_matrix(g, kept[:5])  # 12 haplotypes x 5 sites: the reference's covariance branch
    a, _ = R.transform(x, 9)
    assert a.shape == (12, 5)
    assert np.abs(R.canonical_signs(a) - R.canonical_signs(R.transform_svd(x, 9))).max() <= 1e-11


def test_set_clear_values_are_the_standardised_entries():
    g = cohort(seed=4)
    kept, _ = R.site_filter(g)
    x = R.haplotype_matrix(g, kept)
    hi, lo = R.set_clear_values(x.sum(axis=0), x.shape[0])
    z = R.standardize(x.copy())
    assert np.abs(np.where(x == 1, hi[None, :], lo[None, :]) - z).max() <= 1e-14


# ---- filter known answers -------------------------------------------------------------------------------------------------------
def site_with_count(samples, count):
    row = np.zeros(samples * 2, dtype=np.int16)
    row[:count] = 1
    return row.reshape(samples, 2)


@pytest.mark.parametrize("n,count,kept", [(40, 1, False), (40, 2, True), (40, 38, True), (40, 39, False),
                                           (100, 4, False), (100, 5, True), (100, 95, True), (100, 96, False)])
def test_filter_boundary_maf(n, count, kept):
    g = np.stack([site_with_count(n // 2, count)])
    rows, complete = R.site_filter(g)
    assert complete == 1 and (rows.size == 1) == kept
    assert (20 * min(count, n - count) >= n) == kept  # the exact test agrees with the f64 expression here


def test_filter_missing_multiallelic_and_the_two_complete_counts():
    base = site_with_count(10, 8).astype(np.int16)
    missing = base.copy()
    missing[3, 1] = -1
    multi = base.copy()
    multi[4, 0] = 2
    both = base.copy()
    both[0, 0] = 2
    both[9, 1] = -1
    g = np.stack([base, missing, multi, both, base])
    rows, complete = R.site_filter(g)
    assert rows.tolist() == [0, 4] and complete == 2          # dense input: an allele above 1 is not complete (pca.rs:261-268)
    rows_v, complete_v = R.site_filter(g, variant_rule=True)
    assert rows_v.tolist() == [0, 4] and complete_v == 3      # Variant input: it is complete, then skipped (pca.rs:93-117)
    assert R.clamp_components(10, complete, 20) == 2 and R.clamp_components(10, complete_v, 20) == 3
    assert R.clamp_components(10, 50, 20) == 10 and R.clamp_components(30, 50, 20) == 20


def test_canonical_signs():
    s = np.array([[0.0, -1.0], [-2.0, 3.0], [4.0, 5.0]])
    assert np.array_equal(R.canonical_signs(s), np.array([[0.0, 1.0], [2.0, -3.0], [-4.0, -5.0]]))


# ---- the module's validation needs no device ----------------------------------------------------------------------------------------
def test_validation_errors_without_a_device(fm):
    x = {"genotypes": np.zeros((4, 3, 2), dtype=np.int16), "positions": np.arange(4, dtype=np.int64)}
    names = ["a", "b", "c"]
    with pytest.raises(ValueError, match="sample_names must contain at least one sample"):
        fm.chromosome_pca(x, [], 3)
    with pytest.raises(ValueError, match="n_components must be greater than or equal to 1"):
        fm.chromosome_pca(x, names, 0)
    with pytest.raises(ValueError, match=r"expected diploid genotypes \(ploidy=2\) but received ploidy 3"):
        fm.chromosome_pca({"genotypes": np.zeros((4, 3, 3), dtype=np.int8), "positions": np.arange(4)}, names, 2)
    with pytest.raises(ValueError, match="positions length 5 does not match variant dimension 4"):
        fm.chromosome_pca({"genotypes": np.zeros((4, 3, 2), dtype=np.uint8), "positions": np.arange(5)}, names, 2)
    with pytest.raises(ValueError, match="genotype sample dimension 3 does not match sample_names length 2"):
        fm.chromosome_pca(x, names[:2], 2)
    with pytest.raises(ValueError, match="genotypes must be a numpy.ndarray with dtype int16/int8/uint8/uint16"):
        fm.chromosome_pca({"genotypes": np.zeros((4, 3, 2), dtype=np.float64), "positions": np.arange(4)}, names, 2)
    with pytest.raises(ValueError, match="dense chromosome PCA input requires a 'positions' array"):
        fm.chromosome_pca({"genotypes": np.zeros((4, 3, 2), dtype=np.int8)}, names, 2)
    with pytest.raises(ValueError, match="allele values must fit within signed 16-bit integers"):
        fm.chromosome_pca({"genotypes": np.full((4, 3, 2), 40000, dtype=np.uint16), "positions": np.arange(4)}, names, 2)
    with pytest.raises(ValueError, match="variant 1 contains 2 samples but 3 names were provided"):
        fm.chromosome_pca([(1, [[0, 1], [1, 1], [0, 0]]), (2, [[0, 1], [1, 1]])], names, 2)
    # an empty LIST is the dense form with no variants (lib.rs:1871-1922); any other empty sequence takes the Variant route (pca.rs:57-59)
    with pytest.raises(ValueError, match="No variants with MAF >= 5% found for PCA"):
        fm.chromosome_pca([], names, 2)
    with pytest.raises(ValueError, match="No variants provided for PCA"):
        fm.chromosome_pca((), names, 2)
    # the same order in the file-writing entry points
    with pytest.raises(ValueError, match="sample_names must contain at least one sample"):
        fm.chromosome_pca_to_file([], [], "1", "out", 0)
    with pytest.raises(ValueError, match="n_components must be greater than or equal to 1"):
        fm.per_chromosome_pca({}, names, "out", 0)
    with pytest.raises(ValueError, match="variants_by_chromosome must be a dict"):
        fm.per_chromosome_pca([], names, "out", 2)
    with pytest.raises(NotImplementedError):
        fm.global_pca({}, [], "out")  # unchanged in this version


def test_result_class_is_not_constructible(fm):
    with pytest.raises(TypeError):
        fm.ChromosomePcaResult()


# ---- text -----------------------------------------------------------------------------------------------------------------------
def test_tsv_text_matches_the_reference_format(fm):
    from ferromic import _core

    labels = ["a_L", "a_R", "b_L", "b_R"]
    coords = np.array([[1.5, -2.0000005, 0.0], [1e-9, -1e-9, 123456.7890125], [0.1234565, 0.1234575, -0.0000005], [2.5e-7, 7.5e-7, 1e10]])
    text = _core._pca_tsv_text(labels, coords)
    assert text == R.tsv_text(labels, coords)
    assert text.splitlines()[0] == "Haplotype\tPC1\tPC2\tPC3"
    assert text.splitlines()[1] == "a_L\t1.500000\t-2.000001\t0.000000"  # hand-made: {:.6}
    assert text.splitlines()[2].startswith("a_R\t0.000000\t-0.000000\t")
    assert text.endswith("\n") and text.count("\n") == 5


def test_combine_pca_results(fm, tmp_path):
    from ferromic import _core

    d = tmp_path / "chr_pca"
    d.mkdir()
    (d / "pca_chr_2.tsv").write_text("Haplotype\tPC1\tPC2\ns1_L\t0.100000\t-0.200000\ns1_R\t0.300000\t0.400000\n")
    (d / "pca_chr_10.tsv").write_text("Haplotype\tPC1\tPC2\ns1_L\t1.000000\t2.000000\nbroken-line\ns1_R\t3.000000\t4.000000\n")
    (d / "notes.txt").write_text("ignored\n")
    out = tmp_path / "combined.tsv"
    _core._combine_pca_results(str(d), str(out))
    # file-name order (pca_chr_10 before pca_chr_2), a Chromosome column after the haplotype, lines with fewer than two fields dropped
    assert out.read_text() == ("Haplotype\tChromosome\tPC1\tPC2\n"
                               "s1_L\t10\t1.000000\t2.000000\ns1_R\t10\t3.000000\t4.000000\n"
                               "s1_L\t2\t0.100000\t-0.200000\ns1_R\t2\t0.300000\t0.400000\n")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="No chromosome PCA result files found"):
        _core._combine_pca_results(str(empty), str(out))
    with pytest.raises(ValueError, match="VCF error: Io"):
        _core._combine_pca_results(str(tmp_path / "absent"), str(out))


# ---- the library's host eigen solver ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 17, 200])
def test_host_eigen_solver_against_numpy(fm, n):
    from ferromic import _core

    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n))
    a = (a + a.T) / 2
    w, v = _core._pca_eigen_host(a)
    w0, _ = np.linalg.eigh(a)
    norm = np.abs(w0).max()
    # a backward-stable symmetric solver: eigenvalues, residual and orthogonality at the order of n eps ||A|| (constant 10)
    tol = 10 * n * 2.0 ** -52
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - w0).max() <= tol * norm
    assert np.abs(a @ v - v * w).max() <= tol * norm
    assert np.abs(v.T @ v - np.eye(n)).max() <= tol


def test_host_eigen_solver_on_a_gram_with_repeated_eigenvalues(fm):
    from ferromic import _core

    a = np.diag([1.0, 1.0, 2.0, 0.0, 0.0])
    w, v = _core._pca_eigen_host(a)
    assert np.array_equal(w, np.array([0.0, 0.0, 1.0, 1.0, 2.0]))
    assert np.abs(a @ v - v * w).max() == 0.0
    ones = np.ones((6, 6))
    w, v = _core._pca_eigen_host(ones)
    assert abs(w[-1] - 6.0) <= 1e-14 and np.abs(w[:-1]).max() <= 1e-14
    assert np.abs(np.abs(v[:, -1]) - 1 / np.sqrt(6.0)).max() <= 1e-15
