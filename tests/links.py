"""A few ranks of a large context, any two of them a link (-m gpu).

TEST INFRASTRUCTURE for tests/test_gpu_ranks.py and tests/test_gpu_world20.py:
plain classes and functions, no fixtures.  `Links` attaches the given ranks
(numbers of the caller's choice, lengths per rank) of a context of `nranks`
ranks on GPU 0 with seeded tx; host[r] is what rank r's tx holds.  `round`
runs one call on each of several disjoint links at once, every side on a
thread of its own, and then compares everything a caller can see with host
bytes: each side's results, the WHOLE of every attached rank's rx (the
message, then the 0xEE prefill to the end; all prefill on a rank that did not
call) and tx, and mpx_link_counters of every attached rank towards every rank
number of the context, read before and after: a link that called moved by
the call's iterations and one call, every other row is unchanged.
"""
from __future__ import annotations

import threading

import mpx
import oracle_py as O
import payload

M64 = 0xFFFFFFFFFFFFFFFF
PINGPONG, NONBLOCKING, UNIDIR = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING, mpx.MODE_UNIDIR
PROTO_LL, PROTO_BULK, PROTO_SDMA, PROTO_PULL, PROTO_SDMA_PULL = 0, 1, 2, 7, 8


def link(g1, g0, mode, n, iters, check=True, proto=None, **kw):
    """one call on the link of ranks g1 (group 1) and g0 (group 0); g1 == g0:
    the rank paired with itself (non-blocking only).  kw: mpx.Context.xfer's
    nwg / stream / pull, and armed=True (mpx_xfer_arm first, every armed side
    of the round meets at a barrier, then the call starts it)"""
    return dict(g1=g1, g0=g0, mode=mode, n=n, iters=iters, check=check, proto=proto, kw=kw)


class Links:
    def __init__(self, engine, ranks, cap, nranks=mpx.MAX_RANKS, caps=None):
        self.ranks = list(ranks)
        self.nranks = nranks
        self.caps = {r: (caps or {}).get(r, cap) for r in self.ranks}
        self.c = mpx.Context(nranks, engine)
        self.bufs, self.host = {}, {}
        for r in self.ranks:
            n = self.caps[r]
            tx, rx = self.c.alloc(0, n), self.c.alloc(0, n)
            key = mpx.pattern_key(mpx.PATTERN_SEED, r, 0, 0)
            self.c.fill(tx, n, mpx.FILL_SPLITMIX, key)
            self.c.attach(r, 0, tx, rx, n)
            self.bufs[r] = (tx, rx)
            self.host[r] = O.fill(n, mpx.FILL_SPLITMIX, key)

    def close(self):
        self.c.close()

    def counters(self):
        """every attached rank's row of counters towards every rank number"""
        return {(r, p): self.c.link_counters(r, p) for r in self.ranks for p in range(self.nranks)}

    def advance(self, a, b, seq_by=0, calls_by=0):
        """both sides of the link (a, b) jump forward alike (between calls)"""
        self.c.test_advance_link(a, b, seq_by, calls_by, 0)
        if a != b:
            self.c.test_advance_link(b, a, seq_by, calls_by, 0)

    def sides(self, specs):
        """(spec, rank, peer, group) of every calling side; the links are disjoint"""
        out = []
        for s in specs:
            out.append((s, s["g1"], s["g0"], 1))
            if s["g0"] != s["g1"]:
                out.append((s, s["g0"], s["g1"], 0))
        ranks = [x[1] for x in out]
        assert len(ranks) == len(set(ranks)) and set(ranks) <= set(self.ranks), ranks
        return out

    def start(self, specs, timeout_ms=5000):
        """the calls themselves: rank -> Timing, rank -> MpxError"""
        sides = self.sides(specs)
        out, errs = {}, {}
        bar = threading.Barrier(max(1, sum(1 for s, *_ in sides if s["kw"].get("armed"))))

        def side(s, r, p, g):
            kw = {k: v for k, v in s["kw"].items() if k != "armed"}
            h = self.host[p]
            m = 1 if (s["mode"] == UNIDIR and g == 1) else s["n"]
            exp = dict(expect=O.checksum(h[:s["n"]]), expect_ack=O.checksum(h[:1])) if m <= len(h) else {}
            args = (s["mode"], g, r, p, s["iters"], self.bufs[r][0], self.bufs[r][1], s["n"])
            try:
                if s["kw"].get("armed"):
                    try:
                        self.c.arm(*args, check_payload=s["check"], timeout_ms=timeout_ms, **exp, **kw)
                    finally:
                        bar.wait(timeout=30)
                out[r] = self.c.xfer(*args, check_payload=s["check"], timeout_ms=timeout_ms, **exp, **kw)
            except (mpx.MpxError, threading.BrokenBarrierError) as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=x) for x in sides]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return out, errs

    def round(self, specs, what, timeout_ms=5000):
        for r in self.ranks:
            self.c.fill(self.bufs[r][1], self.caps[r], mpx.FILL_BYTE, payload.GUARD_BYTE)
        before = self.counters()
        out, errs = self.start(specs, timeout_ms)
        assert not errs, (what, errs)
        moved = {}       # (rank, peer) -> iterations
        rx = {r: b"" for r in self.ranks}
        for s, r, p, g in self.sides(specs):
            t, n, iters = out[r], s["n"], s["iters"]
            m = 1 if (s["mode"] == UNIDIR and g == 1) else n
            expected = self.host[p][:m]
            done = O.lib().oracle_nb_waited(iters) if s["mode"] == NONBLOCKING else iters
            assert t.check_failures == 0 and t.check_iters == (iters if s["check"] else 0), (what, r, t.check_iters)
            assert t.recv_done == done, (what, r, t.recv_done)
            if s["check"]:
                assert t.recv_digest == (done * O.checksum(expected)) & M64, (what, r)
            assert t.bytes == n * iters * (1 if s["mode"] == UNIDIR else 2), (what, r, t.bytes)
            if s["proto"] is not None:
                assert t.protocol == s["proto"], (what, r, t.protocol)
            if s["kw"].get("nwg") and t.protocol in (PROTO_BULK, PROTO_PULL):
                assert t.nwg == s["kw"]["nwg"], (what, r, t.nwg)
            moved[(r, p)] = iters
            rx[r] = expected if iters > 0 else b""
        for r in self.ranks:
            want = rx[r] + bytes([payload.GUARD_BYTE]) * (self.caps[r] - len(rx[r]))
            payload.compare(self.c.read(self.bufs[r][1], self.caps[r]), want, 0, f"{what}: rx of rank {r}")
            payload.compare(self.c.read(self.bufs[r][0], self.caps[r]), self.host[r], 0, f"{what}: tx of rank {r}")
        callers = {r for r, _ in moved}
        kernel = self.c.engine == mpx.ENGINE_KERNEL
        for (r, p), b in before.items():
            it = moved.get((r, p))
            want = dict(b, token=b["token"] + (1 if kernel and r in callers else 0))
            if it is not None:
                want.update(tx_seq=b["tx_seq"] + it, rx_seq=b["rx_seq"] + it, calls=b["calls"] + (1 if it > 0 else 0))
            assert self.c.link_counters(r, p) == want, (what, r, p, b, self.c.link_counters(r, p), want)
        return out

    def refused(self, specs, what, status=mpx.ERR_INVALID):
        """every side of these calls is refused with `status` before anything
        moves: no byte of any rx or tx, no counter"""
        for r in self.ranks:
            self.c.fill(self.bufs[r][1], self.caps[r], mpx.FILL_BYTE, payload.GUARD_BYTE)
        before = self.counters()
        out, errs = self.start(specs)
        assert not out and sorted(errs) == sorted(x[1] for x in self.sides(specs)), (what, out, errs)
        for r, e in errs.items():
            assert isinstance(e, mpx.MpxError) and e.status == status, (what, r, e)
        for r in self.ranks:
            payload.compare(self.c.read(self.bufs[r][1], self.caps[r]), bytes([payload.GUARD_BYTE]) * self.caps[r], 0,
                            f"{what}: rx of rank {r}")
            payload.compare(self.c.read(self.bufs[r][0], self.caps[r]), self.host[r], 0, f"{what}: tx of rank {r}")
        assert self.counters() == before, what
