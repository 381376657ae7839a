"""Numpy oracle of the haplotype homozygosity windows, written from the definition in include/ferromic_hip.h and sharing nothing with the
kernel.

A cohort is an allele matrix x [rows][cols] (uint8, alleles 0..7) and a called matrix [rows][cols] (bool) or None = everything called; a
group is a boolean column mask with n members, ranked 0..n-1 by ascending column; a window is a row range [begin, end).  An entry's state is
its allele, or 255 when it is not called.  Two members are identical in a window when their states agree at every row of it - so the
classes are the distinct rows of the [n][rows] state matrix, which np.unique(axis=0) finds.  The statistics are plain Python int / int."""

import numpy as np


def states(x, called):
    return x if called is None else np.where(called, x, 255).astype(np.uint8)


def window(state, members, begin, end):
    """One window: (class sizes sorted descending [K] int64, first [n] int64 = the rank of the first member identical to each member)."""
    n = len(members)
    hap = state[int(begin):int(end)][:, members].T  # [n][rows]
    if hap.shape[1] == 0:
        inverse = np.zeros(n, dtype=np.int64)
    else:
        inverse = np.unique(hap, axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
    sizes = np.bincount(inverse)
    lowest = np.full(sizes.size, n, dtype=np.int64)
    np.minimum.at(lowest, inverse, np.arange(n))
    return np.sort(sizes)[::-1], lowest[inverse]


def windows(x, called, mask, ranges):
    """Every window of `ranges`: dict of sum_sq [w] uint64, distinct [w] uint32, top [w][3] uint32, first [w][n] uint32."""
    members = np.nonzero(np.asarray(mask, dtype=bool))[0]
    n = len(members)
    state = states(x, called)
    out = dict(sum_sq=np.zeros(len(ranges), dtype=np.uint64), distinct=np.zeros(len(ranges), dtype=np.uint32),
               top=np.zeros((len(ranges), 3), dtype=np.uint32), first=np.zeros((len(ranges), n), dtype=np.uint32))
    for w, (begin, end) in enumerate(ranges):
        sizes, first = window(state, members, begin, end)
        out["sum_sq"][w] = sum(int(c) * int(c) for c in sizes)
        out["distinct"][w] = len(sizes)
        out["top"][w, : min(3, len(sizes))] = sizes[:3]
        out["first"][w] = first
    return out


def stats(sum_sq, top, n):
    """The five statistics of one window record, each one division of two Python ints."""
    sum_sq, n = int(sum_sq), int(n)
    c1, c2, c3 = (int(c) for c in top)
    return dict(
        h1=sum_sq / (n * n),
        h12=(sum_sq + 2 * c1 * c2) / (n * n),
        h123=(sum_sq + 2 * (c1 * c2 + c1 * c3 + c2 * c3)) / (n * n),
        h2_h1=(sum_sq - c1 * c1) / sum_sq,
        haplotype_diversity=float("nan") if n == 1 else (n * n - sum_sq) / (n * (n - 1)),
    )
