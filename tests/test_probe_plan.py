"""The probe harness (tests/probe.py) against fake loops driven by a Python
thread: no GPU.  This is where the harness's ability to FAIL is proved — each
broken loop must fail for its own reason, with the stuck range named — and
where the good loop alone stays within the 8 counted / 1 inconclusive mark
the GPU tests (test_gpu_live_copy.py, test_gpu_live_xfer.py) hold libmpx to.
"""
import threading
import time

import numpy as np
import pytest

import probe

G = 64                    # guard bytes either side of the payload
POISON = 0xEE
N = 4096 + 5              # 256 16-B units and a 5-byte tail
DEADLINES = dict(start_deadline_s=2.0, join_deadline_s=10.0, poll_sleep_s=50e-6)


def pattern(k: int, n: int = N) -> np.ndarray:
    """two byte patterns that differ at every offset, neither holding the poison"""
    return ((np.arange(n, dtype=np.uint32) * 7 + 13 + 101 * k) % 199).astype(np.uint8)


class FakeLoop:
    """dst = 64 guard bytes, N payload bytes, 64 guard bytes; src holds
    pattern 0 or 1.  call(): `iters` iterations of about 0.1 ms each, of
    which the first always copies everything; `how` says what the others do."""

    def __init__(self, how: str, iters: int = 3000):
        self.how, self.iters = how, iters
        self.poison_byte = POISON
        self.mem = np.zeros(G + N + G, np.uint8)
        self.k = 0
        self.src = pattern(0)
        self.expected = np.full(G + N + G, POISON, np.uint8)
        self.expected[G:G + N] = self.src
        self.guards = np.ones(G + N + G, bool)
        self.guards[G:G + N] = False
        self.poisons = 0
        self.second_poison = threading.Event()

    # the surface
    def poison(self):
        self.mem[:] = POISON
        self.poisons += 1
        if self.poisons == 2:            # the first probe (the first poison precedes the call)
            self.second_poison.set()

    def snapshot(self):
        return self.mem.copy()

    def rewrite(self):
        self.k ^= 1
        self.src[:] = pattern(self.k)
        self.expected[G:G + N] = self.src

    # the loop
    def call(self):
        dst = self.mem[G:G + N]
        first_load = self.src.copy()
        for it in range(self.iters):
            edge = it == 0 or it == self.iters - 1
            how = "all" if it == 0 else self.how
            if how == "all" or (how == "first_last" and edge):
                dst[:] = self.src
            elif how == "skip_unit":             # unit 100 only in iteration 0
                dst[:1600] = self.src[:1600]
                dst[1616:] = self.src[1616:]
            elif how == "skip_tail":             # the 5 bytes after the last unit only in iteration 0
                dst[:4096] = self.src[:4096]
            elif how == "hoisted":               # stores what it loaded first
                dst[:] = first_load
            elif how == "guard":                 # and one byte past the end
                dst[:] = self.src
                self.mem[G + N] = 0x11
            elif how == "returns":               # gone as soon as the first probe has poisoned
                assert self.second_poison.wait(5.0)
                return "returned"
            time.sleep(50e-6)
        return "done"


def run(loop: FakeLoop, load=False, probe_deadline_s=0.1):
    return probe.run_probed(loop.call, loop, load=load, probe_deadline_s=probe_deadline_s, **DEADLINES)


@pytest.mark.parametrize("load", [False, True])
def test_loop_that_rewrites_everything_counts_its_probes(load):
    loop = FakeLoop("all")
    kinds = ("store", "load") if load else ("store",)
    rep = probe.require(run(loop, load=load, probe_deadline_s=2.0), kinds)
    assert all(rep.counted[k] >= probe.MIN_COUNTED for k in kinds) and rep.inconclusive <= probe.MAX_INCONCLUSIVE
    assert rep.counted["load"] == 0 or load
    assert rep.result == "done" and rep.started_s is not None
    assert "counted" in str(rep) and "inconclusive" in str(rep)


def test_loop_complete_only_in_first_and_last_iteration_is_stuck():
    """the payload never comes back while the call runs: every payload byte is named"""
    with pytest.raises(probe.ProbeError) as e:
        run(FakeLoop("first_last"))
    assert (e.value.reason, e.value.kind) == ("stuck", "store")
    assert (e.value.first, e.value.last, e.value.count) == (G, G + N - 1, N)


def test_loop_complete_only_in_first_and_last_iteration_counts_nothing():
    """the same loop under a deadline longer than the call: its last iteration
    restores the bytes once, as the call returns: one probe at the most"""
    loop = FakeLoop("first_last", iters=300)
    rep = run(loop, probe_deadline_s=5.0)
    assert rep.total <= 1 and rep.inconclusive <= 1
    with pytest.raises(probe.ProbeError) as e:
        probe.require(rep)
    assert e.value.reason == "too_few"


@pytest.mark.parametrize("how,first,count", [("skip_unit", G + 1600, 16), ("skip_tail", G + 4096, 5)])
def test_loop_that_drops_a_range_after_iteration_0_names_it(how, first, count):
    with pytest.raises(probe.ProbeError) as e:
        run(FakeLoop(how))
    assert (e.value.reason, e.value.kind) == ("stuck", "store")
    assert (e.value.first, e.value.last, e.value.count) == (first, first + count - 1, count)
    assert str(first) in str(e.value) and str(first + count - 1) in str(e.value)


def test_loop_that_stores_its_first_loaded_values_fails_the_load_probe_only():
    rep = probe.require(run(FakeLoop("hoisted"), probe_deadline_s=2.0))
    assert rep.counted["store"] >= probe.MIN_COUNTED
    with pytest.raises(probe.ProbeError) as e:
        run(FakeLoop("hoisted"), load=True)
    assert (e.value.reason, e.value.kind, e.value.count) == ("stuck", "load", N)


def test_loop_that_writes_a_guard_byte_fails():
    with pytest.raises(probe.ProbeError) as e:
        run(FakeLoop("guard"))
    assert e.value.reason == "guard" and (e.value.first, e.value.last, e.value.count) == (G + N, G + N, 1)


def test_call_that_returns_during_the_first_probe_is_inconclusive():
    rep = run(FakeLoop("returns"))
    assert rep.total == 0 and rep.inconclusive == 1 and rep.result == "returned"
    assert rep.overtaken == ("store", str(0), str(G + N + G - 1), G + N + G) or rep.overtaken[3] == N
    assert "still missed" in str(rep)
    with pytest.raises(probe.ProbeError) as e:
        probe.require(rep)
    assert e.value.reason == "too_few"
    rep.inconclusive = 2
    with pytest.raises(probe.ProbeError) as e:
        probe.require(rep)
    assert e.value.reason == "inconclusive"


def test_call_that_never_writes_has_not_started():
    loop = FakeLoop("all")
    loop.call = lambda: time.sleep(0.3)
    with pytest.raises(probe.ProbeError) as e:
        probe.run_probed(loop.call, loop, start_deadline_s=0.05, probe_deadline_s=0.05, join_deadline_s=5.0,
                         poll_sleep_s=50e-6)
    assert e.value.reason == "not_started" and e.value.count == N


def test_the_calls_own_error_is_raised_and_the_worker_joined():
    loop = FakeLoop("all")

    def call():
        raise ValueError("the call failed")

    before = threading.active_count()
    with pytest.raises(ValueError):
        probe.run_probed(call, loop, probe_deadline_s=0.1, **DEADLINES)
    assert threading.active_count() == before


def test_wrong_bytes_after_the_call_fail():
    """complete while probed, wrong at the end (the last iteration breaks one byte)"""
    loop = FakeLoop("all", iters=600)
    inner = loop.call

    def call():
        inner()
        loop.mem[G + 7] ^= 0x40
        return "done"

    with pytest.raises(probe.ProbeError) as e:
        probe.run_probed(call, loop, probe_deadline_s=2.0, **DEADLINES)
    assert e.value.reason == "final" and (e.value.first, e.value.count) == (G + 7, 1)


def test_joined_surfaces_count_together_and_name_the_part():
    good, bad = FakeLoop("all"), FakeLoop("skip_unit")

    def call():
        t = threading.Thread(target=bad.call)
        t.start()
        good.call()
        t.join()

    both = probe.Joined([("rank 0 rx", good), ("rank 1 rx", bad)])
    with pytest.raises(probe.ProbeError) as e:
        probe.run_probed(call, both, probe_deadline_s=0.1, **DEADLINES)
    assert e.value.reason == "stuck" and e.value.first == (G + N + G) + G + 1600 and e.value.count == 16
    assert f"rank 1 rx + {G + 1600}" in str(e.value)
    a, b = FakeLoop("all"), FakeLoop("all")

    def call2():
        t = threading.Thread(target=b.call)
        t.start()
        a.call()
        t.join()

    probe.require(probe.run_probed(call2, probe.Joined([("a", a), ("b", b)]), probe_deadline_s=2.0, **DEADLINES))


def test_size_iters():
    """0.4 s from a 2000-iteration call, never fewer than that call, within int"""
    assert probe.size_iters(2000 * 2e-6) == 200000          # 2 us per iteration
    assert probe.size_iters(1.0) == probe.SIZING_ITERS       # already longer than the target
    assert probe.size_iters(0.0) == probe.INT_MAX
    assert probe.size_iters(2000 * 1e-6, target_s=0.1) == 100000
