"""run_vcf --pca without a GPU: which variants, samples and alleles the chromosome PCA takes (`--ingest_only --pca` prints a digest
of the diploid PASS matrix, compared with the oracle's parse), the three flags, the TSV writer that the Python module and run_vcf
now share, and the C-ABI symbol of the sharded Gram."""

import os
import re
import subprocess

import numpy as np
import pytest

from tests import pca_ref as R
from tests.pca_vcf_helpers import diploid_entries, make_mixed_cohort, oracle_pass_variants, pca_input_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("FERROMIC_RUN_VCF_BIN") or os.path.join(ROOT, "ferromic_amd", "bin", "run_vcf")
ENV = dict(os.environ, FERROMIC_PROGRESS="0", FERROMIC_THREADS="3")
PCA_LINE = re.compile(r"\[PCA_INPUT\] chr (\S+): (\d+) variants x (\d+) samples digest ([0-9a-f]{16})")


def base_cmd(kw, tmp_path):
    return [BIN, "--vcf_folder", kw["vcf_folder"], "--reference", kw["reference"], "--gtf", kw["gtf"], "--output_file", str(tmp_path / "out" / "o.csv")]


def pca_lines(stdout):
    return {m.group(1): (int(m.group(2)), int(m.group(3)), m.group(4)) for m in PCA_LINE.finditer(stdout)}


@pytest.mark.parametrize("variant", ["plain", "mask_allow_exclude_gq"])
def test_pca_input_matches_the_oracle_parse(tmp_path, variant):
    kw, names = make_mixed_cohort(tmp_path, seed=301 if variant == "plain" else 302)
    cmd = base_cmd(kw, tmp_path) + ["--config_file", kw["config_file"], "--ingest_only", "--pca"]
    opts = {}
    if variant != "plain":
        cmd += ["--mask_file", str(tmp_path / "mask.bed"), "--allow_file", str(tmp_path / "allow.tsv"), "--min_gq", "31", "--exclude", names[4]]
        opts = dict(min_gq=31, mask_file=str(tmp_path / "mask.bed"), allow_file=str(tmp_path / "allow.tsv"), exclude=[names[4]])
    res = subprocess.run(cmd, capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = pca_lines(res.stdout)
    exp = {}
    incomplete = high = 0
    for c, (variants, sample_names) in oracle_pass_variants(kw, **opts).items():
        exp[c] = (len(variants), len(sample_names), pca_input_digest(variants, len(sample_names)))
        g = diploid_entries(variants, len(sample_names))
        incomplete += int((g < 0).any(axis=(1, 2)).sum())
        high += int((g > 1).any(axis=(1, 2)).sum())
        assert names[4] not in sample_names or variant == "plain"
    assert got == exp and set(got) == {"1", "7", "X"}, (got, exp)
    assert all(v[0] > 20 for v in exp.values()), exp        # the digest covers real matrices ...
    assert incomplete > 10 and high > 10, (incomplete, high)  # ... with haploid cells and multi-allelic sites among the PASS variants
    assert res.stdout.count("[INGEST] chr") == 3              # the ingest lines are still there


def test_without_pca_nothing_is_printed(tmp_path):
    kw, _ = make_mixed_cohort(tmp_path, seed=303)
    res = subprocess.run(base_cmd(kw, tmp_path) + ["--config_file", kw["config_file"], "--ingest_only"], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode == 0 and "[PCA_INPUT]" not in res.stdout and "pca" not in res.stderr.lower(), res.stderr[-500:]
    assert not (tmp_path / "pca_per_chr_outputs").exists()


def test_single_chromosome_mode_digest(tmp_path):
    kw, _ = make_mixed_cohort(tmp_path, seed=304)
    res = subprocess.run(base_cmd(kw, tmp_path) + ["--chr", "7", "--region", "200-3000", "--ingest_only", "--pca"], capture_output=True, text=True,
                         env=ENV, timeout=300, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    variants, sample_names = oracle_pass_variants(kw, chrom="7", region="200-3000")["7"]
    assert pca_lines(res.stdout) == {"7": (len(variants), len(sample_names), pca_input_digest(variants, len(sample_names)))}
    assert not (tmp_path / "pca_per_chr_outputs").exists()  # --ingest_only computes nothing


def test_pca_flags(tmp_path):
    kw, _ = make_mixed_cohort(tmp_path, seed=305)
    cmd = base_cmd(kw, tmp_path) + ["--config_file", kw["config_file"], "--ingest_only", "--pca"]
    plain = subprocess.run(cmd, capture_output=True, text=True, env=ENV, timeout=300)
    assert plain.returncode == 0 and "ignored" not in plain.stderr, plain.stderr[-500:]  # the old warning is gone
    for extra in (["--pca_components", "4"], ["--pca_components=25", "--pca_output", "somewhere.tsv"], ["--pca_output=x"], ["--pca_components", "+3"]):
        res = subprocess.run(cmd + extra, capture_output=True, text=True, env=ENV, timeout=300)
        assert res.returncode == 0 and pca_lines(res.stdout) == pca_lines(plain.stdout), (extra, res.stderr[-500:])
    for bad in ("four", "-1", "2.5", ""):
        res = subprocess.run(cmd + ["--pca_components", bad], capture_output=True, text=True, env=ENV, timeout=300)
        assert res.returncode != 0 and "--pca_components" in res.stderr, (bad, res.stderr[-300:])
    res = subprocess.run(cmd + ["--pca_components"], capture_output=True, text=True, env=ENV, timeout=300)
    assert res.returncode != 0
    text = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--pca " in text and "--pca_components" in text and "--pca_output" in text and "pca_per_chr_outputs" in text


def test_module_tsv_writer_is_byte_identical():
    """The writer moved into the header run_vcf shares: same bytes as the restatement, for values that exercise {:.6}."""
    from ferromic import _core

    rng = np.random.default_rng(7)
    coords = rng.normal(scale=30.0, size=(24, 5))
    coords[0] = [0.0, -0.0, 1e-7, -4.9999995e-7, 123456.7890125]
    coords[1] = [0.5e-6, 1.5e-6, -2.5e-6, 1e15, -1e-300]
    labels = [f"s{i}_{side}" for i in range(12) for side in "LR"]
    assert _core._pca_tsv_text(labels, coords) == R.tsv_text(labels, coords)
    assert _core._pca_tsv_text(labels[:3], coords[:3, :1]) == R.tsv_text(labels[:3], coords[:3, :1])
    assert _core._pca_tsv_text([], np.zeros((0, 2))) == "Haplotype\tPC1\tPC2\n"


def test_sharded_gram_symbol_is_declared_exported_and_prototyped():
    import ctypes as C

    from ferromic_amd import _abi

    header = open(os.path.join(ROOT, "include", "ferromic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+fmh_pca_gram_sharded\s*\(\s*fmh_comm\s*\*", code)
    assert "fmh_pca_gram_sharded" in _abi.SYMBOLS and len(_abi.SYMBOLS["fmh_pca_gram_sharded"][1]) == 8
    lib = C.CDLL(os.path.join(ROOT, "ferromic_amd", "lib", "libferromic_hip.so"))
    assert hasattr(lib, "fmh_pca_gram_sharded")
    assert lib.fmh_abi_version() == 3  # additive
    # argument checks need no device: NULL handles are refused before anything else
    fn = _abi.load().fmh_pca_gram_sharded
    assert fn(None, None, None, 0, None, None, None, None) == _abi.FMH_ERR_INVALID
