"""fmh_pca_gram_sharded: the PCA Gram of a cohort whose sites are spread over the ranks of a communicator (ranks as host threads
over one device: the in-process transport; one-rank local and RCCL communicators).

Entry by entry against Z Z^T / (n - 1) over ALL kept sites with the derived bound of tests/test_gpu_pca.py, where (m + 2) becomes
(m + 2 + R): the R per-rank Grams are each divided (R divisions instead of one) and added (R - 1 more additions); m = kept sites
over all ranks.  Exactly symmetric, every rank the same bits, two calls the same bits."""

import ctypes as C
import threading
import time

import numpy as np
import pytest

from tests import pca_ref as R
from tests.test_gpu_pca import EPS, binary_rows

pytestmark = pytest.mark.gpu


def run_ranks(ranks, work):
    out, errors = [None] * ranks, []

    def call(r):
        try:
            out[r] = work(r)
        except Exception as exc:  # noqa: BLE001 - reported by the main thread
            errors.append((r, exc))

    threads = [threading.Thread(target=call, args=(r,)) for r in range(ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in threads), "a rank is still inside the collective"
    return out, errors


def cohort(n, rows, ranks, seed, empty_rank):
    """x, the slab cuts (uneven), the kept rows (sorted, with holes, none inside slab `empty_rank`) and their set / clear values."""
    rng = np.random.default_rng(seed)
    x = binary_rows(rng, rows, n)
    inner = np.sort(rng.choice(np.arange(70, rows - 70), size=ranks - 1, replace=False)) if ranks > 1 else np.array([], dtype=np.int64)
    cuts = [0] + [int(c) for c in inner] + [rows]
    candidates = np.arange(3, rows)
    if empty_rank is not None:
        candidates = candidates[(candidates < cuts[empty_rank]) | (candidates >= cuts[empty_rank + 1])]
    kept = np.sort(rng.choice(candidates, size=min(candidates.size - 5, (2 * rows) // 3), replace=False)).astype(np.int64)
    hi, lo = R.set_clear_values(x[kept].sum(axis=1), n)
    return x, cuts, kept, hi, lo


@pytest.mark.parametrize("layout", ["packed", "bytes"])
@pytest.mark.parametrize("n", [6, 130, 1002])
@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_sharded_gram_entry_by_entry(fmh_opts, ranks, n, layout):
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    rows = 1100
    empty_rank = None if ranks == 1 else ranks - 2
    x, cuts, kept, hi, lo = cohort(n, rows, ranks, 7000 + 10 * n + ranks, empty_rank)
    m = kept.size
    z = np.where(x[kept].T == 1, hi[None, :], lo[None, :])
    expected = z @ z.T / float(n - 1)
    bound = 2.0 * (m + 2 + ranks) * EPS * (np.abs(z) @ np.abs(z).T) / float(n - 1)
    if layout == "bytes":
        fmh_opts.setenv("FMH_LAYOUT", "bytes")
    # one rank: the RCCL communicator a one-GPU box allows (pack -> ncclAllReduce -> unpack); more: the in-process transport
    comms = sharding.Comm.init_all([0] * ranks) if ranks > 1 else [sharding.Comm.single(0)]
    try:
        def work(r):
            b, e = cuts[r], cuts[r + 1]
            mine = (kept >= b) & (kept < e)
            dm = dev.DeviceMatrix.from_host(x[b:e], None, e - b, n // 2, 2, 1)
            try:
                first = dev.pca_gram_sharded(comms[r], dm, kept[mine] - b, hi[mine], lo[mine])
                again = dev.pca_gram_sharded(comms[r], dm, kept[mine] - b, hi[mine], lo[mine])
            finally:
                dm.close()
            return first, again, int(mine.sum())

        out, errors = run_ranks(ranks, work)
        assert not errors, errors
    finally:
        for c in comms:
            c.close()
    if empty_rank is not None:
        assert out[empty_rank][2] == 0 and sum(o[2] for o in out) == m
        assert len({o[2] for o in out}) > 1  # uneven
    for r in range(ranks):
        got, again, _ = out[r]
        err = np.abs(got - expected)
        worst = float((err / bound).max())
        print(f"sharded gram R={ranks} n={n} m={m} layout={layout} rank {r}: max err {err.max():.3e}, max err/bound {worst:.3e}")
        assert np.all(err <= bound), (ranks, n, layout, r, worst)
        assert np.array_equal(got, got.T), "the Gram must be exactly symmetric"
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "two calls must give the same bits"
        assert np.array_equal(got.view(np.uint64), out[0][0].view(np.uint64)), "every rank must leave with the same bits"


@pytest.mark.parametrize("n,m", [(6, 63), (130, 4097), (1002, 300)])
def test_world_of_one_equals_the_plain_gram(n, m):
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    rng = np.random.default_rng(n + m)
    rows = m + 40
    x = binary_rows(rng, rows, n)
    kept = np.sort(rng.choice(np.arange(2, rows), size=m, replace=False)).astype(np.uint64)
    hi, lo = R.set_clear_values(x[kept.astype(np.int64)].sum(axis=1), n)
    dm = dev.DeviceMatrix.from_host(x, None, rows, n // 2, 2, 1)
    try:
        plain = dev.pca_gram(dm, kept, hi, lo)
        for comm, transport in ((sharding.Comm.local(0), "local"), (sharding.Comm.single(0), "rccl")):
            assert (comm.world, comm.transport) == (1, transport)
            got = dev.pca_gram_sharded(comm, dm, kept, hi, lo)
            assert np.array_equal(got.view(np.uint64), plain.view(np.uint64)), transport
            zeros = dev.pca_gram_sharded(comm, dm, [], [], [])
            assert zeros.shape == (n, n) and not zeros.any(), transport
            comm.close()
    finally:
        dm.close()


def test_argument_errors_return_before_the_collective(fmh_opts):
    """On a two-rank in-process group only rank 0 calls: had a refused call entered the collective it would wait for rank 1 for ever."""
    from ferromic_amd import _abi
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    lib = _abi.load()
    n, m = 130, 65
    rng = np.random.default_rng(3)
    x = binary_rows(rng, 100, n)
    kept = np.arange(10, 10 + m, dtype=np.uint64)
    hi, lo = R.set_clear_values(x[10:10 + m].sum(axis=1), n)
    comms = sharding.Comm.init_all([0, 0])
    dm = dev.DeviceMatrix.from_host(x, None, 100, n // 2, 2, 1)
    tri = dev.DeviceMatrix.from_host(np.zeros((4, 6), dtype=np.uint8), None, 4, 2, 3, 1)  # ploidy 3
    results = {}

    def only_rank_zero():
        d = dev.DeviceBuffer(0, 8 * n * n)
        results["null comm"] = lib.fmh_pca_gram_sharded(None, dm._h, kept.ctypes.data_as(C.c_void_p), m, hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), d.ptr, None)
        results["null gram"] = lib.fmh_pca_gram_sharded(comms[0]._h, dm._h, kept.ctypes.data_as(C.c_void_p), m, hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), None, None)
        results["null rows"] = lib.fmh_pca_gram_sharded(comms[0]._h, dm._h, None, m, hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), d.ptr, None)
        for key, call, match in (
            ("ploidy", lambda: dev.pca_gram_sharded(comms[0], tri, [0], [1.0], [0.0]), "ploidy"),
            ("row", lambda: dev.pca_gram_sharded(comms[0], dm, [100], [1.0], [0.0]), "exceeds"),
        ):
            try:
                call()
                results[key] = "no error"
            except _abi.FerromicHipError as exc:
                results[key] = match in str(exc)
        # the Gram alone fits this budget (135 200 + 8 192 + 4 096 + 520 bytes), the packed triangle (68 120 bytes) on top does not
        fmh_opts.setenv("FMH_PCA_BUDGET_BYTES", "150000")
        results["plain fits"] = dev.pca_gram(dm, kept, hi, lo).shape == (n, n)
        results["budget"] = (lib.fmh_pca_gram_sharded(comms[0]._h, dm._h, kept.ctypes.data_as(C.c_void_p), m, hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), d.ptr, None),
                             lib.fmh_last_error())

    t = threading.Thread(target=only_rank_zero)
    t.start()
    t.join(timeout=120)
    try:
        assert not t.is_alive(), f"a refused call entered the collective: {results}"
        assert results["null comm"] == results["null gram"] == results["null rows"] == _abi.FMH_ERR_INVALID, results
        assert results["ploidy"] is True and results["row"] is True and results["plain fits"] is True, results
        assert results["budget"][0] == _abi.FMH_ERR_UNSUPPORTED and b"FMH_PCA_BUDGET_BYTES" in results["budget"][1], results
    finally:
        if t.is_alive():
            comms[1].abort()
            t.join(timeout=30)
        dm.close()
        tri.close()
        for c in comms:
            c.close()


def test_different_sample_counts_are_an_error_not_a_wrong_sum():
    from ferromic_amd import _abi
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    comms = sharding.Comm.init_all([0, 0])

    def work(r):
        n = (6, 8)[r]
        x = binary_rows(np.random.default_rng(r), 20, n)
        hi, lo = R.set_clear_values(x.sum(axis=1), n)
        dm = dev.DeviceMatrix.from_host(x, None, 20, n // 2, 2, 1)
        try:
            with pytest.raises(_abi.FerromicHipError, match="different sample counts"):
                dev.pca_gram_sharded(comms[r], dm, np.arange(20), hi, lo)
        finally:
            dm.close()
        return True

    out, errors = run_ranks(2, work)
    for c in comms:
        c.close()
    assert not errors and out == [True, True], errors


def test_abort_wakes_the_ranks_waiting_for_the_gram():
    """Rank 1 "fails" before its call and aborts (the library's abort call, as run_vcf's slab threads do): ranks 0 and 2, waiting in the
    rendezvous with their triangles, return an error instead of hanging, and the group refuses every later collective."""
    from ferromic_amd import _abi
    from ferromic_amd import device as dev
    from ferromic_amd import sharding

    n = 130
    comms = sharding.Comm.init_all([0, 0, 0])
    results = {}

    def waiter(r):
        x = binary_rows(np.random.default_rng(r), 80, n)
        hi, lo = R.set_clear_values(x.sum(axis=1), n)
        dm = dev.DeviceMatrix.from_host(x, None, 80, n // 2, 2, 1)
        try:
            dev.pca_gram_sharded(comms[r], dm, np.arange(80), hi, lo)
            results[r] = "returned a Gram"
        except _abi.FerromicHipError as exc:
            results[r] = str(exc)
        finally:
            dm.close()

    threads = [threading.Thread(target=waiter, args=(r,)) for r in (0, 2)]
    for t in threads:
        t.start()
    time.sleep(2.0)  # both have their local Gram and wait for rank 1
    assert all(t.is_alive() for t in threads), results
    comms[1].abort()
    for t in threads:
        t.join(timeout=30)
    assert not any(t.is_alive() for t in threads), "peers still blocked after fmh_comm_abort"
    for r in (0, 2):
        assert "aborted by rank 1" in results[r], results
    x = binary_rows(np.random.default_rng(9), 10, n)
    dm = dev.DeviceMatrix.from_host(x, None, 10, n // 2, 2, 1)
    with pytest.raises(_abi.FerromicHipError, match="aborted"):
        dev.pca_gram_sharded(comms[0], dm, [0], [1.0], [-1.0])
    dm.close()
    for c in comms:
        c.close()
