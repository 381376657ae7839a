"""numpy oracle of the banded r^2 and the LD pruning of include/ferromic_hip.h (fmh_ld_band, fmh_ld_prune).

It shares no algebra with the kernel: the four counts of every pair come from exact 0/1 float64 MATRIX PRODUCTS
(nAB = A A^T, nA = A C^T, nB = its transpose, n = C C^T; every entry is an integer far below 2^53), the band is read out of them, and
r^2 is the header's formula in numpy int64 / float64 - three roundings, no fused multiply-add, so the device value is these bits.
The greedy rule is plain Python.
"""

import numpy as np


def indicator_matrices(alleles, called=None, column_mask=None):
    """alleles [S][H] integers, called [S][H] bool or None (everything called), column_mask [H] bool or None -> (A, C) float64 0/1:
    C = called & mask, A = (allele >= 1) & C."""
    alleles = np.asarray(alleles)
    S, H = alleles.shape
    c = np.ones((S, H), dtype=bool) if called is None else np.asarray(called, dtype=bool).copy()
    if column_mask is not None:
        c &= np.asarray(column_mask, dtype=bool)[None, :]
    a = (alleles >= 1) & c
    return a.astype(np.float64), c.astype(np.float64)


def r2_from_counts(n, nA, nB, nAB):
    n, nA, nB, nAB = (np.asarray(x, dtype=np.int64) for x in (n, nA, nB, nAB))
    D = n * nAB - nA * nB
    vA, vB = nA * (n - nA), nB * (n - nB)
    ok = (vA != 0) & (vB != 0)
    num = D.astype(np.float64) * D.astype(np.float64)
    den = vA.astype(np.float64) * vB.astype(np.float64)
    out = np.full(n.shape, np.nan, dtype=np.float64)
    np.divide(num, den, out=out, where=ok)
    return out


def band(alleles, called, column_mask, row_begin, row_count, partner_end, band, threshold, block=512):
    """What fmh_ld_band writes for rows [row_begin, row_begin + row_count): dict of r2 / n_ab / n_joint [rows][band], over
    [rows][ceil(band / 32)] uint32, site_n / site_alt [rows].  Entries whose partner is not below partner_end: NaN, 0, bit 0."""
    A, C = indicator_matrices(alleles, called, column_mask)
    words = (band + 31) // 32
    r2 = np.full((row_count, band), np.nan, dtype=np.float64)
    n_ab = np.zeros((row_count, band), dtype=np.uint32)
    n_joint = np.zeros((row_count, band), dtype=np.uint32)
    for b0 in range(0, row_count, block):
        rows = np.arange(row_begin + b0, row_begin + min(b0 + block, row_count))
        p0, p1 = int(rows[0]) + 1, min(int(rows[-1]) + band + 1, partner_end)
        if p1 <= p0:
            continue
        Ai, Ci, Aj, Cj = A[rows], C[rows], A[p0:p1], C[p0:p1]
        m_ab, m_a, m_b, m_n = Ai @ Aj.T, Ai @ Cj.T, (Aj @ Ci.T).T, Ci @ Cj.T  # [rows][partners], exact integers
        j = rows[:, None] + np.arange(1, band + 1)[None, :]
        valid = j < partner_end
        col = np.where(valid, j - p0, 0)
        take = lambda mtx: np.rint(np.take_along_axis(mtx, col, axis=1)).astype(np.int64)
        k_ab, k_a, k_b, k_n = take(m_ab), take(m_a), take(m_b), take(m_n)
        sl = slice(b0, b0 + len(rows))
        r2[sl] = np.where(valid, r2_from_counts(k_n, k_a, k_b, k_ab), np.nan)
        n_ab[sl] = np.where(valid, k_ab, 0)
        n_joint[sl] = np.where(valid, k_n, 0)
    with np.errstate(invalid="ignore"):
        bits = r2 > threshold  # NaN never exceeds
    padded = np.zeros((row_count, words * 32), dtype=np.uint8)
    padded[:, :band] = bits
    over = np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(row_count, words) if row_count else np.zeros((0, words), np.uint32)
    rows_all = slice(row_begin, row_begin + row_count)
    return dict(r2=r2, n_ab=n_ab, n_joint=n_joint, over=over.astype(np.uint32),
                site_n=C[rows_all].sum(axis=1).astype(np.uint32), site_alt=A[rows_all].sum(axis=1).astype(np.uint32))


def greedy_from_r2(r2, threshold):
    """The forward greedy rule over a [rows][window] r^2 band whose partners end with the rows."""
    rows, window = r2.shape
    keep = [True] * rows
    for i in range(rows):
        if not keep[i]:
            continue
        for d in range(1, window + 1):
            j = i + d
            if j >= rows:
                break
            v = r2[i, d - 1]
            if v > threshold:  # False for NaN
                keep[j] = False
    return np.array(keep, dtype=bool)


def greedy_from_bits(over, band_width):
    """The same rule over threshold bits [rows][ceil(band / 32)] (bit (d - 1) & 31 of word (d - 1) >> 5)."""
    over = np.asarray(over, dtype=np.uint32)
    rows = over.shape[0]
    keep = [True] * rows
    for i in range(rows):
        if not keep[i]:
            continue
        for d in range(1, band_width + 1):
            j = i + d
            if j >= rows:
                break
            if (int(over[i, (d - 1) >> 5]) >> ((d - 1) & 31)) & 1:
                keep[j] = False
    return np.array(keep, dtype=bool)
