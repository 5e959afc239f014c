"""Fan exchange: matched-receive order across calls, independence of a rank's
links, and the phases a call reports (-m gpu, MI355X; loopback ranks on GPU 0).

* rx read between calls: the scenario of tests/ordering.py (race) on fan
  links.  Every rank runs call 1 (pattern A); the racing ranks rewrite their
  tx (pattern B) and enter call 2 at once; one rank sleeps RACE_DELAY_S, reads
  its WHOLE rx on the host and must find exactly call 1's blocks, 0xEE
  elsewhere; then it calls, and after call 2 everything holds pattern B.
  Workgroup (k, 0) posts the link's call number and no workgroup pushes
  before it has read the peer's post: that is what holds the racers back.
  The negative control runs the same scenario under MPX_TEST=no_posted and
  must see call 2's bytes in the sleeper's rx.
* link independence: a star whose leaf 2 calls D = 0.5 s late.  Leaf 1's call
  must return, and the hub's link to leaf 1 must end, long before leaf 2 has
  called; the hub's link to leaf 2 and its kernel must last beyond D / 2.
  Both thresholds follow from the injected sleep, not from a measurement.
* phases: what mpx_last_phases holds after a fan call.

Every expectation is host bytes (tests/fan.py).  The racing ranks write tx
with mpx_fill (the context's utility stream): a host copy on the null stream
could wait for the peers' kernels, which wait for this rank.
"""
import threading
import time

import pytest

import mpx
import oracle_py as O
import payload
from fan import Fan, flat_image, full_mesh, round16
from ordering import RACE_DELAY_S

pytestmark = pytest.mark.gpu

N = 65555
ITERS = 3
SEED_B = 1


def race(nranks: int, check: bool):
    """-> (what the sleeper read between the calls, what call 1 must have
    left there).  The last rank sleeps; every other rank races."""
    sets = full_mesh(nranks)
    sleeper = nranks - 1
    F = Fan(nranks, nranks * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        F.prefill()
        stride = F.stride
        A = list(F.host)
        B = [flat_image(F.cap, r, SEED_B) for r in range(nranks)]
        want_between = F.expected_rx(sleeper, sets[sleeper])
        res, errs, out2 = {}, {}, {}

        def sums(img, r):
            return [O.checksum(img[p][r * stride:r * stride + N]) for p in sets[r]]

        def side(r):
            tx, rx = F.bufs[r]
            try:
                F.c.fan(r, sets[r], ITERS, tx, rx, N, stride, check_payload=check, expect=sums(A, r), timeout_ms=5000)
                if r == sleeper:
                    time.sleep(RACE_DELAY_S)
                    res["between"] = F.c.read(rx, F.cap)
                F.fill_tx(r, SEED_B)
                out2[r] = F.c.fan(r, sets[r], ITERS, tx, rx, N, stride, check_payload=check, expect=sums(B, r),
                                  timeout_ms=5000)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,)) for r in range(nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs                 # (the racers' call 2 succeeds once the sleeper calls)
        F.host = B
        F.verify(sets, out2, ITERS, check, ("after call 2", nranks, check), widths=5)
        return res["between"], want_between
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("nranks", [2, 3])
def test_rx_read_between_calls(nranks, check):
    between, want = race(nranks, check)
    payload.compare(between, want, 0, f"rx of the sleeping rank between the calls ({nranks} ranks, check {check})")


def test_rx_read_between_calls_fails_without_the_handshake(monkeypatch):
    """Negative control, in a context of its own with MPX_TEST=no_posted for
    the whole test (FanLink.call = 0: every wait for the post holds at once).
    Without check mode a racer pushes all of call 2 and waits only for the
    sleeper's last flag, so nothing times out: its call ends once the sleeper
    calls.  The sleeper's rx then holds call 2's bytes after 0.3 s, and the
    comparison the positive test makes must raise."""
    monkeypatch.setenv("MPX_TEST", "no_posted")
    between, want = race(2, False)
    with pytest.raises(AssertionError, match="bytes differ, first at offset"):
        payload.compare(between, want, 0, "rx between the calls, no handshake")
    B0 = flat_image(len(want), 0, SEED_B)
    assert between[:N] == B0[round16(N):round16(N) + N]       # exactly the racer's new block, early


D = 0.5
STAR = {0: [1, 2], 1: [0], 2: [0]}


@pytest.mark.parametrize("check", [True, False])
def test_one_late_link_does_not_hold_the_other(check):
    F = Fan(3, 3 * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        F.checked_call(STAR, ITERS, check, "warm-up", widths=5)      # tables and checksum arrays allocated
        F.prefill()
        out, errs, stamp = {}, {}, {}

        def side(r):
            exp = [O.checksum(F.block(p, r)) for p in STAR[r]]
            if r == 2:
                time.sleep(D)
            stamp[r, "call"] = time.monotonic()
            try:
                out[r] = F.c.fan(r, STAR[r], ITERS, F.bufs[r][0], F.bufs[r][1], N, F.stride, check_payload=check,
                                 expect=exp, timeout_ms=5000)
            except mpx.MpxError as e:
                errs[r] = e
            stamp[r, "return"] = time.monotonic()
            if r == 0:
                stamp["phases"] = F.c.phases(0)

        th = [threading.Thread(target=side, args=(r,)) for r in STAR]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        F.verify(STAR, out, ITERS, check, ("late leaf", check), widths=5)
        # leaf 1 was done while leaf 2 had not called
        assert stamp[1, "return"] < stamp[2, "call"], stamp
        assert out[1][0].wall_s < D / 2, out[1][0].wall_s
        hub = {l["peer"]: l["device_s"] for l in out[0][1]}
        assert hub[1] < D / 2 < hub[2], hub
        assert stamp["phases"]["kernel_s"] > D / 2, stamp["phases"]
        assert out[1][1][0]["device_s"] < D / 2, out[1][1]
    finally:
        F.close()


RING4 = {0: [1, 3], 1: [2, 0], 2: [3, 1], 3: [0, 2]}
STAR4 = {0: [3, 1, 2], 1: [0], 2: [0], 3: [0]}


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("shape", ["mesh3", "ring4", "star4"])
def test_phases_after_a_fan_call(shape, check):
    """mpx_last_phases after a fan call: the call's own wall time; the post
    wait and the tail lie inside the kernel's span; every link's end is
    stamped before the call's exit stamp, on one clock; and the kernel's 10 ns
    tick against the host clock keeps the floor tests/test_gpu_lat.py asserts"""
    n, sets = {"mesh3": (3, full_mesh(3)), "ring4": (4, RING4), "star4": (4, STAR4)}[shape]
    F = Fan(n, n * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        F.prefill()
        got, errs = {}, {}

        def side(r):
            exp = [O.checksum(F.block(p, r)) for p in sets[r]]
            try:
                t, links = F.c.fan(r, sets[r], 17, F.bufs[r][0], F.bufs[r][1], N, F.stride, check_payload=check,
                                   expect=exp, timeout_ms=5000)
                got[r] = (t, links, F.c.phases(r))     # the rank's own thread: no later call of its has run
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,)) for r in sets]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        F.verify(sets, {r: g[:2] for r, g in got.items()}, 17, check, ("phases", shape, check), widths=5)
        for r, (t, links, ph) in got.items():
            what = (shape, check, r, ph, links)
            assert ph["wall_s"] == t.wall_s, what
            assert ph["kernel_s"] > 0, what
            assert 0 <= ph["posted_wait_s"] <= ph["kernel_s"], what
            assert 0 <= ph["tail_s"] <= ph["kernel_s"], what
            assert all(0 <= l["device_s"] <= ph["kernel_s"] + 1e-8 for l in links), what
            assert 0.98 * ph["kernel_s"] <= ph["wall_s"], what
            assert ph["armed"] == 0, what
    finally:
        F.close()
