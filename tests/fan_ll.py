"""Loopback ranks for the lock-step LL fan tests (tests/test_gpu_fan_ll.py and
its worker tests/fan_ll_worker.py, -m gpu).

TEST INFRASTRUCTURE: tests/fan.py's Fan with every call made with
MPX_FAN_LL (F.ll = False: a bulk fan call on the same links) and what such a
call reports: protocol 10, one workgroup per link, everything else as for a
bulk fan call.  Every expectation is host bytes, as in tests/fan.py.
"""
from __future__ import annotations

import threading
import time

import mpx
import oracle_py as O
import payload
from fan import M64, Fan, flat_image, full_mesh, round16

PROTO_FAN_LL = 10
LL_MAX = 4096


class LLFan(Fan):
    ll = True

    def run(self, peersets, iters, check=True, timeout_ms=5000, prefill=True, late=None, **kw):
        if self.ll:
            kw.setdefault("ll", True)
        return super().run(peersets, iters, check=check, timeout_ms=timeout_ms, prefill=prefill, late=late, **kw)

    def verify(self, peersets, out, iters, check, what, widths=None):
        if not self.ll:
            return super().verify(peersets, out, iters, check, what, widths=widths)
        self.verify_bytes(peersets, what, moved=iters > 0)
        for r, peers in peersets.items():
            t, links = out[r]
            k = len(peers)
            assert t.protocol == PROTO_FAN_LL == mpx.PROTO_FAN_LL, (what, r, t.protocol)
            assert t.launches == 1 and t.nwg == 1, (what, r, t.launches, t.nwg)
            assert t.bytes == 2 * self.block_len * iters * k, (what, r, t.bytes)
            assert t.recv_done == k * iters, (what, r, t.recv_done)
            sums = [O.checksum(self.block(p, r)) for p in peers]
            assert t.recv_digest == (sum(iters * s for s in sums) & M64 if check else 0), (what, r)
            assert t.check_failures == 0 and t.check_iters == (k * iters if check else 0), (what, r, t.check_iters)
            assert [l["peer"] for l in links] == list(peers), (what, r)
            for j, l in enumerate(links):
                assert l["nwg"] == 1 and l["recv_done"] == iters and l["check_failures"] == 0, (what, r, l)
                assert l["recv_digest"] == ((iters * sums[j]) & M64 if check else 0), (what, r, l)
                assert 0 <= l["device_s"] < 5.0, (what, r, l)


def mesh(nranks: int, n: int, stride: int = 0) -> LLFan:
    stride = stride or max(16, round16(n))
    F = LLFan(nranks, nranks * stride + payload.GUARD)
    F.layout(n, stride)
    return F


# ---- rx read between two calls (tests/test_gpu_fan_order.py race, on LL calls) --
RACE_N, RACE_ITERS, RACE_DELAY_S, SEED_B = 4096, 3, 0.3, 1


def race(nranks: int, check: bool, second_ll: bool = True):
    """Every rank runs call 1 (LL, pattern A, an odd number of iterations: call
    2's first push lands in the other half of the row than call 1's first).
    The racing ranks rewrite their tx (pattern B) and enter call 2 at once; the
    last rank sleeps, reads its WHOLE rx and only then rewrites and calls.
    second_ll = False: call 2 is a bulk fan call, whose pushes go straight into
    the peer's rx.  -> (what the sleeper read between the calls, what call 1
    must have left there)."""
    sets = full_mesh(nranks)
    sleeper = nranks - 1
    F = mesh(nranks, RACE_N)
    try:
        F.prefill()
        stride = F.stride
        A = list(F.host)
        B = [flat_image(F.cap, r, SEED_B) for r in range(nranks)]
        want_between = F.expected_rx(sleeper, sets[sleeper])
        res, errs, out2 = {}, {}, {}

        def sums(img, r):
            return [O.checksum(img[p][r * stride:r * stride + RACE_N]) for p in sets[r]]

        def side(r):
            tx, rx = F.bufs[r]
            try:
                F.c.fan(r, sets[r], RACE_ITERS, tx, rx, RACE_N, stride, check_payload=check, expect=sums(A, r),
                        timeout_ms=5000, ll=True)
                if r == sleeper:
                    time.sleep(RACE_DELAY_S)
                    res["between"] = F.c.read(rx, F.cap)
                F.fill_tx(r, SEED_B)
                out2[r] = F.c.fan(r, sets[r], RACE_ITERS, tx, rx, RACE_N, stride, check_payload=check, expect=sums(B, r),
                                  timeout_ms=5000, ll=second_ll)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,)) for r in range(nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        F.host = B
        F.ll = second_ll
        F.verify(sets, out2, RACE_ITERS, check, ("after call 2", nranks, check, second_ll))
        for r, p in ((a, b) for a in range(nranks) for b in range(nranks) if a != b):
            c = F.counters(r, p)
            assert c["tx_seq"] == c["rx_seq"] == 2 * RACE_ITERS and c["calls"] == 2, (r, p, c)
        return res["between"], want_between
    finally:
        F.close()
