"""Run a handful of callables from host threads that start every round together, and say what happened: which worker failed in which
round, which one never came back, and whether any two calls were in flight at the same time at all.

A worker is (name, call, check): call() makes one library call (or the two or three that belong together) and returns what it got, check(result)
asserts on it.  Whatever check compares with is computed by the test on the main thread before run_workers is entered - the oracles are slow and
they are the thing compared against, so no thread ever computes one.

What the harness does not do: it never repeats a call, never loops until something shows, and never runs more than MAX_THREADS threads.  The
rounds are a fixed small number.  After the first failure no thread starts another call."""

import threading
import time
import traceback
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

MAX_THREADS = 8


@dataclass
class Failure:
    worker: str
    round: int      # counted from 1
    error: BaseException
    trace: str


@dataclass
class Hang:
    worker: str
    round: int      # the round the thread was in when timeout_s ran out
    where: str      # "call", "check" or "barrier": what had not returned


@dataclass
class Report:
    rounds: int
    failures: List[Failure] = field(default_factory=list)
    hangs: List[Hang] = field(default_factory=list)
    overlaps: List[int] = field(default_factory=list)   # per round: pairs of calls of different workers whose host intervals intersect
    calls: Dict[str, int] = field(default_factory=dict)  # per worker: calls started

    def assert_ok(self):
        """No failure, no hang, every round ran and had two calls in flight at once."""
        lines = [f"{f.worker} failed in round {f.round}: {f.error!r}\n{f.trace}" for f in self.failures]
        lines += [f"{h.worker} hung in round {h.round} ({h.where})" for h in self.hangs]
        assert not lines, "\n".join(lines)
        assert len(self.overlaps) == self.rounds, self.overlaps
        # a condition, not a measurement: a binding that kept the interpreter lock would make every concurrent test vacuous
        assert all(count > 0 for count in self.overlaps), f"no two calls overlapped in some round: {self.overlaps}"


def count_overlaps(intervals: Sequence[Tuple[int, float, float]]) -> int:
    """Pairs of (thread, begin, end) intervals of different threads that intersect."""
    count = 0
    for i, (ti, b0, e0) in enumerate(intervals):
        for tj, b1, e1 in intervals[i + 1:]:
            if ti != tj and max(b0, b1) < min(e0, e1):
                count += 1
    return count


def run_workers(workers: Sequence[Tuple[str, Callable, Callable]], rounds: int, timeout_s: float,
                serialize: Optional[threading.Lock] = None) -> Report:
    """One daemon thread per worker; a barrier releases them together at the start of each of the `rounds` rounds.  `timeout_s` bounds the whole
    run: a thread that has not finished by then is reported as a hang - with the round it was in and whether in its call or its check - and left
    behind.  `serialize` (the harness's own test) takes that lock
    around every timed call, which is what a binding that kept the interpreter lock would amount to: the overlap counts must then be 0."""
    if not 1 <= len(workers) <= MAX_THREADS:
        raise ValueError(f"1 to {MAX_THREADS} workers, got {len(workers)}")
    if rounds < 1:
        raise ValueError("at least one round")
    n = len(workers)
    report = Report(rounds=rounds, calls={name: 0 for name, _, _ in workers})
    stop = threading.Event()
    barrier = threading.Barrier(n)
    guard = threading.Lock()
    intervals: List[List[Tuple[int, float, float]]] = [[] for _ in range(rounds)]
    at: List[Tuple[int, str]] = [(0, "barrier")] * n   # (round from 1, "barrier" | "call" | "check"): where each thread is

    def fail(idx, rnd, error):
        with guard:
            report.failures.append(Failure(workers[idx][0], rnd, error, traceback.format_exc()))
        stop.set()
        barrier.abort()

    def body(idx):
        name, call, check = workers[idx]
        for rnd in range(1, rounds + 1):
            at[idx] = (rnd, "barrier")
            try:
                barrier.wait()
            except threading.BrokenBarrierError:
                return
            if stop.is_set():
                return
            try:
                with guard:
                    report.calls[name] += 1
                at[idx] = (rnd, "call")
                if serialize is not None:
                    with serialize:
                        begin = time.perf_counter()
                        result = call()
                        end = time.perf_counter()
                else:
                    begin = time.perf_counter()
                    result = call()
                    end = time.perf_counter()
                at[idx] = (rnd, "check")
                with guard:
                    intervals[rnd - 1].append((idx, begin, end))
                check(result)
            except BaseException as error:  # noqa: BLE001 - an assertion, a library error, anything: it ends the run
                fail(idx, rnd, error)
                return

    threads = [threading.Thread(target=body, args=(i,), name=f"worker-{workers[i][0]}", daemon=True) for i in range(n)]
    deadline = time.monotonic() + timeout_s
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        stop.set()
        barrier.abort()  # whoever waits for the missing thread leaves now
        for idx, t in enumerate(threads):
            if at[idx][1] == "barrier":   # released by the abort: gone in a moment
                t.join(1.0)
        for idx, t in enumerate(threads):
            if t.is_alive():
                report.hangs.append(Hang(workers[idx][0], *at[idx]))
    with guard:
        finished = [r for r in range(rounds) if len(intervals[r]) == n]
        report.overlaps = [count_overlaps(intervals[r]) for r in finished]
    return report
