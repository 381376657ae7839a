"""tests/concurrent_harness.py on plain Python callables (no GPU): the harness can fail.  It names the worker and the round of a wrong answer and
of an exception, stops the other workers after the first failure, reports a call that never returns and comes back itself, counts calls that
overlap, and counts none when every call runs under one lock."""

import threading
import time

import pytest

from tests.concurrent_harness import MAX_THREADS, count_overlaps, run_workers

NAP = 0.05   # long against a thread switch, short against the suite


def napper(log=None):
    def call():
        if log is not None:
            log.append(time.perf_counter())
        time.sleep(NAP)
        return 7
    return call


def expect_seven(result):
    assert result == 7


def test_a_wrong_answer_in_round_two_is_named():
    seen = []

    def call():
        seen.append(len(seen) + 1)
        time.sleep(NAP)
        return 7 if len(seen) < 2 else 8

    report = run_workers([("steady", napper(), expect_seven), ("drifts", call, expect_seven)], rounds=3, timeout_s=20)
    assert [(f.worker, f.round) for f in report.failures] == [("drifts", 2)]
    assert isinstance(report.failures[0].error, AssertionError) and not report.hangs
    with pytest.raises(AssertionError, match="drifts failed in round 2"):
        report.assert_ok()


def test_after_an_exception_nobody_calls_again():
    tries = []

    def boom():
        tries.append(1)
        if len(tries) == 2:
            raise RuntimeError("status 2")
        time.sleep(NAP)
        return 7

    logs = [[], []]
    workers = [("a", napper(logs[0]), expect_seven), ("boom", boom, expect_seven), ("b", napper(logs[1]), expect_seven)]
    report = run_workers(workers, rounds=4, timeout_s=20)
    assert [(f.worker, f.round) for f in report.failures] == [("boom", 2)] and "status 2" in report.failures[0].trace
    # the failed call was not repeated; of the others, whoever had looked at the flag before it was set finished round 2, and nobody
    # started round 3 or 4
    assert report.calls["boom"] == 2 and len(tries) == 2
    for name, log in (("a", logs[0]), ("b", logs[1])):
        assert report.calls[name] == len(log) and 1 <= len(log) <= 2, (name, log)
    assert len(report.overlaps) == 1   # round 1 alone was finished by everybody
    with pytest.raises(AssertionError, match="boom failed in round 2"):
        report.assert_ok()


def test_a_call_that_never_returns_is_reported_as_a_hang():
    release = threading.Event()
    rounds_seen = []

    def stuck():
        rounds_seen.append(1)
        if len(rounds_seen) == 2:
            release.wait(30)   # far beyond timeout_s: the harness must not wait for it
        return 7

    began = time.monotonic()
    try:
        report = run_workers([("fine", napper(), expect_seven), ("stuck", stuck, expect_seven)], rounds=3, timeout_s=0.5)
        assert time.monotonic() - began < 5
        assert [(h.worker, h.round, h.where) for h in report.hangs] == [("stuck", 2, "call")] and not report.failures
        assert report.calls == {"fine": 2, "stuck": 2}   # round 3 never started
        with pytest.raises(AssertionError, match="stuck hung in round 2"):
            report.assert_ok()
    finally:
        release.set()


def test_a_check_that_never_returns_is_reported_with_its_round():
    release = threading.Event()
    checks = []

    def stuck_check(result):
        checks.append(1)
        if len(checks) == 2:
            release.wait(30)

    try:
        report = run_workers([("fine", napper(), expect_seven), ("slow-check", napper(), stuck_check)], rounds=3, timeout_s=0.5)
        assert [(h.worker, h.round, h.where) for h in report.hangs] == [("slow-check", 2, "check")] and not report.failures
        with pytest.raises(AssertionError, match=r"slow-check hung in round 2 \(check\)"):
            report.assert_ok()
    finally:
        release.set()


def test_sleeping_calls_overlap():
    workers = [(f"w{i}", napper(), expect_seven) for i in range(4)]
    report = run_workers(workers, rounds=3, timeout_s=20)
    report.assert_ok()
    assert len(report.overlaps) == 3 and all(count > 0 for count in report.overlaps)
    assert report.calls == {f"w{i}": 3 for i in range(4)}


def test_under_one_lock_nothing_overlaps():
    workers = [(f"w{i}", napper(), expect_seven) for i in range(4)]
    report = run_workers(workers, rounds=3, timeout_s=20, serialize=threading.Lock())
    assert report.overlaps == [0, 0, 0] and not report.failures and not report.hangs
    with pytest.raises(AssertionError, match="no two calls overlapped"):
        report.assert_ok()


def test_overlap_count_and_thread_cap():
    # same thread: never a pair; touching ends do not intersect
    assert count_overlaps([(0, 0.0, 1.0), (0, 0.5, 1.5), (1, 1.0, 2.0)]) == 1
    assert count_overlaps([(0, 0.0, 1.0), (1, 1.0, 2.0)]) == 0
    assert count_overlaps([(0, 0.0, 3.0), (1, 1.0, 2.0), (2, 1.5, 4.0)]) == 3
    with pytest.raises(ValueError):
        run_workers([(f"w{i}", napper(), expect_seven) for i in range(MAX_THREADS + 1)], rounds=1, timeout_s=1)
