"""Mid-call probes: watch a buffer from outside while ONE call rewrites it
`iters` times (tests/test_probe_plan.py, test_gpu_live_copy.py,
test_gpu_live_xfer.py).

TEST INFRASTRUCTURE: pure Python and numpy, no GPU, no fixtures.

Every hot loop of libmpx runs all its iterations inside one launch, and every
iteration moves the same bytes into the same place, so a test that looks at
the buffers after the call sees the last iteration only.  A probe looks while
the call runs:

  store probe   the whole observed region is overwritten with a poison byte,
                then polled until every payload byte is back;
  load probe    the SOURCE is rewritten with another pattern, then the region
                is polled until it holds the new pattern.

A probe COUNTS if the region is complete (payload as expected, every other
byte still poison) and the call had not returned when that snapshot was read —
the returned flag is looked at after the snapshot.  The bytes that came back
can only have been written after the poison (or the rewrite), so a counted
probe is proof that the loop was still moving every byte at that moment.  A
probe overtaken by the call's return is INCONCLUSIVE and ends the probing.  A
probe still incomplete at its deadline with the call still running FAILS, and
so does a byte other than poison where nothing may be written.

A surface is any object with
    poison_byte   the poison value
    poison()      overwrite the whole observed region with poison_byte
    snapshot()    the whole observed region now, a uint8 array
    expected      uint8 array of that length: the region once complete (the
                  payload where the loop writes, poison_byte elsewhere)
    guards        bool array of that length: True where nothing may write
    rewrite()     (load probes only) give the source its other pattern and
                  update `expected` to match
    locate(off)   (optional) a name for offset `off` of the region
Every deadline is the caller's; nothing here waits unboundedly, and the worker
thread is always joined.
"""
from __future__ import annotations

import threading
import time

import numpy as np

INT_MAX = (1 << 31) - 1
MIN_COUNTED = 8          # counted probes a case needs, of every kind it uses
MAX_INCONCLUSIVE = 1     # and at most this many inconclusive ones (the last)
SIZING_ITERS = 2000      # the short unprobed call a case is sized from
TARGET_S = 0.4           # about this long per probed call


def size_iters(sizing_wall_s: float, sizing_iters: int = SIZING_ITERS, target_s: float = TARGET_S) -> int:
    """iterations that make a call of this shape last about target_s, from the
    wall time of a call of sizing_iters; within [sizing_iters, INT_MAX].
    Sizing only: a mis-sized call counts too few probes and fails for that."""
    per = max(sizing_wall_s, 1e-9) / sizing_iters
    return int(min(max(target_s / per, sizing_iters), INT_MAX))


class ProbeError(AssertionError):
    """reason: not_started | stuck | guard | too_few | inconclusive | final |
    not_joined; kind: the probe's kind (store / load / start); first, last,
    count: the offsets of the first and last wrong byte and how many are"""

    def __init__(self, reason: str, text: str, kind: str = "", first: int = -1, last: int = -1, count: int = 0,
                 report=None):
        super().__init__(f"{reason}: {text}" + (f" [{report}]" if report is not None else ""))
        self.reason, self.kind, self.first, self.last, self.count, self.report = reason, kind, first, last, count, report


class Worker:
    """the call on a thread of its own; `returned` is set the moment the call
    is back (its result or exception kept), before anything else happens"""

    def __init__(self, fn):
        self.fn = fn
        self.returned = False
        self.result = None
        self.error = None
        self.t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        try:
            self.result = self.fn()
        except BaseException as e:  # noqa: BLE001 (handed to the caller by join)
            self.error = e
        finally:
            self.returned = True

    def start(self):
        self.t.start()

    def join(self, deadline_s: float):
        """the call's result; raises what the call raised"""
        self.t.join(deadline_s)
        if self.t.is_alive():
            raise ProbeError("not_joined", f"the call did not return within {deadline_s} s")
        if self.error is not None:
            raise self.error
        return self.result


class Report:
    def __init__(self):
        self.counted = {"store": 0, "load": 0}
        self.inconclusive = 0
        self.started_s = None      # call start -> first complete payload
        self.probing_s = 0.0
        self.iters = None          # the caller's: the sized iteration count
        self.overtaken = None      # (kind, first, last, count): what the probe the return overtook still missed
        self.result = None         # what the call returned

    @property
    def total(self) -> int:
        return sum(self.counted.values())

    def __str__(self):
        return (f"iters {self.iters}, counted {self.total} (store {self.counted['store']}, load "
                f"{self.counted['load']}), inconclusive {self.inconclusive}, first payload after "
                f"{-1 if self.started_s is None else round(self.started_s * 1e3, 3)} ms, probed for "
                f"{round(self.probing_s * 1e3, 1)} ms" + ("" if self.overtaken is None else
                "; the {} probe that the return overtook still missed {} bytes, {} to {}".format(
                    self.overtaken[0], self.overtaken[3], self.overtaken[1], self.overtaken[2])))


def _wrong(snap: np.ndarray, surface):
    """(offsets of payload bytes not as expected, offsets of guard bytes not poison)"""
    bad = snap != surface.expected
    g = surface.guards
    return np.flatnonzero(bad & ~g), np.flatnonzero(bad & g)


def _name(surface, off: int) -> str:
    loc = getattr(surface, "locate", None)
    return f"{off} ({loc(off)})" if loc else str(off)


def _stuck(reason, kind, surface, idx, what, report) -> ProbeError:
    first, last = int(idx[0]), int(idx[-1])
    return ProbeError(reason, f"{what}: {len(idx)} bytes, first at offset {_name(surface, first)}, last at "
                              f"{_name(surface, last)}", kind, first, last, len(idx), report)


def _await_complete(surface, worker, kind, deadline_s, poll_sleep_s, report):
    """poll until the region is complete: "counted" if the call had not
    returned by then, "inconclusive" if it had (complete or not); raises
    ProbeError for a touched guard at once and for payload still missing at
    the deadline"""
    t0 = time.monotonic()
    while True:
        snap = surface.snapshot()
        returned = worker.returned          # after the snapshot
        miss, touched = _wrong(snap, surface)
        if len(touched):
            raise _stuck("guard", kind, surface, touched, "bytes written where nothing may be", report)
        if not len(miss):
            return "inconclusive" if returned else "counted"
        if returned:
            report.overtaken = (kind, _name(surface, int(miss[0])), _name(surface, int(miss[-1])), len(miss))
            return "inconclusive"
        if time.monotonic() - t0 > deadline_s:
            what = f"{kind} probe not complete after {deadline_s} s with the call still running"
            raise _stuck("not_started" if kind == "start" else "stuck", kind, surface, miss, what, report)
        if poll_sleep_s is not None:
            time.sleep(poll_sleep_s)


def run_probed(call, surface, *, start_deadline_s: float, probe_deadline_s: float, join_deadline_s: float,
               load: bool = False, poll_sleep_s: float | None = 0.0, max_probes: int = 1 << 20, iters=None) -> Report:
    """Poison the region, start call() on a worker thread, wait for the first
    complete payload, then probe back to back until the call returns: store
    probes, alternating with load probes where `load`.  Then the final state:
    exactly `expected` if no probe was overtaken by the return, else every
    byte either as expected or as the overtaken probe left it.  The worker is
    joined on every path.  Returns the Report (Report.result: call()'s);
    raises ProbeError — see require() for the counts."""
    assert poll_sleep_s is None or poll_sleep_s <= 1e-3
    rep = Report()
    rep.iters = iters          # for the report only
    surface.poison()
    left = np.full(len(surface.expected), surface.poison_byte, np.uint8)   # what the last probe's write left
    worker = Worker(call)
    t_call = time.monotonic()
    worker.start()
    failure = None
    try:
        if _await_complete(surface, worker, "start", start_deadline_s, poll_sleep_s, rep) == "counted":
            rep.started_s = time.monotonic() - t_call
            t_probe = time.monotonic()
            kinds = ("store", "load") if load else ("store",)
            for k in range(max_probes):
                if worker.returned:
                    break
                kind = kinds[k % len(kinds)]
                if kind == "store":
                    surface.poison()
                    left = np.full(len(surface.expected), surface.poison_byte, np.uint8)
                else:
                    left = surface.expected.copy()
                    surface.rewrite()
                if _await_complete(surface, worker, kind, probe_deadline_s, poll_sleep_s, rep) == "counted":
                    rep.counted[kind] += 1
                else:
                    rep.inconclusive += 1
                    break
            rep.probing_s = time.monotonic() - t_probe
        else:
            rep.inconclusive += 1      # the call was over before its first payload was seen
    except ProbeError as e:
        failure = e
    try:
        rep.result = worker.join(join_deadline_s)
    except ProbeError:
        raise
    except BaseException:
        if failure is None:
            raise
    if failure is not None:
        raise failure
    snap = surface.snapshot()
    ok = snap == surface.expected
    if rep.inconclusive:
        ok |= (snap == left) & ~surface.guards
    if not ok.all():
        raise _stuck("final", "final", surface, np.flatnonzero(~ok), "wrong bytes after the call", rep)
    return rep


def require(rep: Report, kinds=("store",), min_counted: int = MIN_COUNTED,
            max_inconclusive: int = MAX_INCONCLUSIVE) -> Report:
    """the pass mark: at least min_counted counted probes of every kind used,
    at most max_inconclusive inconclusive ones"""
    if rep.inconclusive > max_inconclusive:
        raise ProbeError("inconclusive", f"{rep.inconclusive} inconclusive probes, at most {max_inconclusive} allowed",
                         report=rep)
    for kind in kinds:
        if rep.counted[kind] < min_counted:
            raise ProbeError("too_few", f"{rep.counted[kind]} counted {kind} probes, {min_counted} needed", kind,
                             report=rep)
    return rep


def say(request, capsys, text: str) -> None:
    """a case's figures: in the captured output always (shown with a
    failure), and under -v on the terminal too, after the test's name"""
    print(text)
    if request.config.getoption("verbose") > 0:
        with capsys.disabled():
            print("\n    " + text, end=" ")


class Joined:
    """several surfaces observed as one: a probe poisons all of them and
    counts when all are complete.  parts: [(name, surface), ...]"""

    def __init__(self, parts):
        self.parts = list(parts)
        self.poison_byte = self.parts[0][1].poison_byte
        assert all(s.poison_byte == self.poison_byte for _, s in self.parts)
        self.starts = np.cumsum([0] + [len(s.expected) for _, s in self.parts])
        self.expected = np.concatenate([s.expected for _, s in self.parts])
        self.guards = np.concatenate([s.guards for _, s in self.parts])

    def poison(self):
        for _, s in self.parts:
            s.poison()

    def snapshot(self):
        return np.concatenate([s.snapshot() for _, s in self.parts])

    def locate(self, off: int) -> str:
        k = int(np.searchsorted(self.starts, off, side="right")) - 1
        name, s = self.parts[k]
        inner = off - int(self.starts[k])
        loc = getattr(s, "locate", None)
        return f"{name} + {inner}" + (f", {loc(inner)}" if loc else "")
