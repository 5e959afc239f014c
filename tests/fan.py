"""Loopback ranks for the fan-exchange tests (tests/test_gpu_fan.py and
tests/test_gpu_fan_{wrap,order,shapes,soak}.py, -m gpu).

TEST INFRASTRUCTURE: plain classes and functions, no fixtures.  N ranks on
GPU 0, one host thread per rank and call, every expectation from host bytes:
host[r] is what rank r's tx holds (block d, for rank d, seeded with the key of
(r, d); the bytes between blocks seeded too, so a push that read the wrong
place shows), rx is 0xEE before every call, and after it the WHOLE of rx and
of tx is read back and compared byte for byte.
"""
from __future__ import annotations

import threading
import time

import mpx
import oracle_py as O
import payload

M64 = 0xFFFFFFFFFFFFFFFF
PROTO_FAN = 9
MIN_PUSH_CHUNK = payload.MIN_PUSH_CHUNK


def pair_nwg(n: int, same_device: bool = True) -> int:
    """bulk_nwg (mpx_internal.h): the pair rule's width"""
    per = (16 << 10) if same_device else (32 << 10)
    return max(1, min(128, -(-n // per)))


def fan_width(nranks: int, n: int, same_device: bool = True, nwg: int = 0, env: int = 0) -> int:
    """the width of a fan link, restated: the call's option, else MPX_FAN_WG,
    else min(pair rule, max(1, 128 // (nranks - 1))); then at least
    kMinPushChunk bytes per workgroup and at least one workgroup"""
    w = nwg if nwg > 0 else env if env > 0 else min(pair_nwg(n, same_device), max(1, 128 // (nranks - 1)))
    return max(1, min(w, -(-n // MIN_PUSH_CHUNK)))


def round16(n: int) -> int:
    return (n + 15) & ~15


def full_mesh(n: int) -> dict:
    return {r: [p for p in range(n) if p != r] for r in range(n)}


def block_bytes(src: int, dst: int, n: int, seed: int = 0) -> bytes:
    """the block rank src sends rank dst under tx seed `seed` (seed 0: the
    bytes Fan.layout has always written)"""
    return O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, src, dst, 7 + 16 * seed))


def tx_image(cap: int, nranks: int, r: int, block_len: int, stride: int, seed: int = 0) -> bytes:
    """the whole of rank r's tx: block d (for rank d) at d * stride, seeded per
    (r, d); the bytes between blocks seeded too"""
    h = bytearray(O.fill(cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 63, 1 + 16 * seed)))
    for d in range(nranks):
        h[d * stride:d * stride + block_len] = block_bytes(r, d, block_len, seed)
    return bytes(h)


def flat_key(r: int, seed: int) -> int:
    return mpx.pattern_key(mpx.PATTERN_SEED, r, 62, seed & 0xFFFFFF)


def flat_image(cap: int, r: int, seed: int) -> bytes:
    """rank r's tx after Fan.fill_tx(r, seed): one seeded stream over the whole
    buffer (block d is its bytes at d * stride), which the device can write on
    the context's utility stream while other ranks' kernels are in flight"""
    return O.fill(cap, mpx.FILL_SPLITMIX, flat_key(r, seed))


def links_of(peersets: dict) -> list:
    """the unordered links (r, p), r < p, of a symmetric peer graph"""
    out = sorted({(min(r, p), max(r, p)) for r, ps in peersets.items() for p in ps})
    assert all(a in peersets.get(b, []) and b in peersets.get(a, []) for a, b in out), peersets
    return out


class Fan:
    """ranks: the ranks attached, of the context's nranks (default: all of
    them); caps: rank -> attached length where it is not cap"""

    def __init__(self, nranks: int, cap: int, engine="kernel", ranks=None, caps=None):
        self.n = nranks
        self.ranks = list(range(nranks)) if ranks is None else list(ranks)
        self.cap = cap
        self.caps = {r: (caps or {}).get(r, cap) for r in self.ranks}
        self.c = mpx.Context(nranks, engine)
        self.bufs = {}
        self.host = [b""] * nranks      # by rank number; a rank not attached holds nothing
        self.block_len = self.stride = 0
        self.seed = 0
        for r in self.ranks:
            n = self.caps[r]
            tx, rx = self.c.alloc(0, n), self.c.alloc(0, n)
            self.c.attach(r, 0, tx, rx, n)
            self.bufs[r] = (tx, rx)

    def close(self):
        self.c.close()

    def layout(self, block_len: int, stride: int) -> None:
        """every rank's tx, written from the host for this block layout"""
        assert self.n * stride <= self.cap and block_len <= stride
        self.block_len, self.stride = block_len, stride
        for r in self.ranks:     # (a rank attached shorter holds the front of the image)
            self.host[r] = tx_image(self.cap, self.n, r, block_len, stride, self.seed)[:self.caps[r]]
            payload.write(self.c, self.bufs[r][0], self.host[r])

    def set_tx_seed(self, k: int) -> None:
        """the same layout from another seed: every byte of every rank's tx
        (blocks and gaps) is drawn anew, so the next call's bytes differ from
        the last call's everywhere"""
        assert k != self.seed
        old = list(self.host)
        self.seed = k
        self.layout(self.block_len, self.stride)
        if self.block_len >= 16:
            for r in self.ranks:
                for d in self.ranks:
                    assert self.block(r, d) != old[r][d * self.stride:d * self.stride + self.block_len], (r, d)

    def fill_tx(self, r: int, seed: int) -> None:
        """rank r's own tx = flat_image(cap, r, seed), written by the device
        (mpx_fill, the utility stream): safe while peers are inside a call.
        self.host is the caller's to update once no thread reads it."""
        self.c.fill(self.bufs[r][0], self.caps[r], mpx.FILL_SPLITMIX, flat_key(r, seed))

    def block(self, src: int, dst: int) -> bytes:
        """what src sends dst"""
        return self.host[src][dst * self.stride:dst * self.stride + self.block_len]

    def prefill(self) -> None:
        for r in self.ranks:
            self.c.fill(self.bufs[r][1], self.caps[r], mpx.FILL_BYTE, payload.GUARD_BYTE)

    def run(self, peersets: dict, iters: int, check=True, timeout_ms=5000, prefill=True, late=None, **kw):
        """peersets: rank -> its peers, in the order it lists them; every
        listed rank calls on a thread of its own.  late: rank -> seconds; such
        a rank sleeps, reads its whole rx (self.rx_before[r]) and only then
        calls, and every rank reads its whole rx the moment its own call
        returns (self.rx_at_return[r]), whatever its peers are doing then."""
        if prefill:
            self.prefill()
        out, errs = {}, {}
        self.rx_before, self.rx_at_return = {}, {}

        def side(r):
            exp = [O.checksum(self.block(p, r)) for p in peersets[r]]
            if late and r in late:
                time.sleep(late[r])
                self.rx_before[r] = self.c.read(self.bufs[r][1], self.caps[r])
            try:
                out[r] = self.c.fan(r, peersets[r], iters, self.bufs[r][0], self.bufs[r][1], self.block_len, self.stride,
                                    check_payload=check, expect=exp, timeout_ms=timeout_ms, **kw)
            except mpx.MpxError as e:
                errs[r] = e
            if late is not None:
                self.rx_at_return[r] = self.c.read(self.bufs[r][1], self.caps[r])

        th = [threading.Thread(target=side, args=(r,)) for r in peersets]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return out, errs

    def late_call(self, peersets: dict, iters: int, check: bool, late: dict, what, widths=None, **kw):
        """checked_call with some ranks entering the call late.  Until a late
        rank calls nothing may land in its rx (it still holds the prefill),
        and no rank that exchanges with it can be done: such a rank's call
        lasts at least half the sleep — a bound that follows from the injected
        delay, not from a measurement — and its rx is complete the moment its
        call returns, not merely by the time every thread has joined."""
        def call():
            out, errs = self.run(peersets, iters, check=check, late=late, **kw)
            assert not errs, (what, errs)
            for r in late:
                blank = bytes([payload.GUARD_BYTE]) * self.caps[r]
                payload.compare(self.rx_before[r], blank, 0, f"{what}: rx of late rank {r} before its call")
            for r, peers in peersets.items():
                payload.compare(self.rx_at_return[r], self.expected_rx(r, peers, iters > 0), 0,
                                f"{what}: rx of rank {r} when its call returned")
                waits = [late[p] for p in peers if p in late and r not in late]
                if waits and iters > 0:
                    assert out[r][0].wall_s > max(waits) / 2, (what, r, out[r][0].wall_s)
            self.verify(peersets, out, iters, check, what, widths=widths)
            return out
        return self.counted(peersets, iters, call)

    def expected_rx(self, r: int, peers, moved=True) -> bytes:
        want = bytearray([payload.GUARD_BYTE]) * self.caps[r]
        if moved:
            for p in peers:
                want[p * self.stride:p * self.stride + self.block_len] = self.block(p, r)
        return bytes(want)

    def verify_bytes(self, peersets: dict, what, moved=True) -> None:
        """rx whole (the peers' blocks, 0xEE everywhere else: the gaps, the
        rank's own block, the blocks of ranks outside the set) and tx whole"""
        for r in self.ranks:
            peers = peersets.get(r, [])
            payload.compare(self.c.read(self.bufs[r][1], self.caps[r]), self.expected_rx(r, peers, moved), 0,
                            f"{what}: rx of rank {r}")
            payload.compare(self.c.read(self.bufs[r][0], self.caps[r]), self.host[r], 0, f"{what}: tx of rank {r}")

    def verify(self, peersets: dict, out: dict, iters: int, check: bool, what, widths=None) -> None:
        """the bytes, and everything the call reports: per link and in total"""
        self.verify_bytes(peersets, what, moved=iters > 0)
        for r, peers in peersets.items():
            t, links = out[r]
            k = len(peers)
            assert t.protocol == PROTO_FAN and mpx.PROTOCOLS[t.protocol] == "fan", (what, r, t.protocol)
            assert t.launches == 1, (what, r)
            assert t.bytes == 2 * self.block_len * iters * k, (what, r, t.bytes)
            assert t.recv_done == k * iters, (what, r, t.recv_done)
            sums = [O.checksum(self.block(p, r)) for p in peers]
            assert t.recv_digest == (sum(iters * s for s in sums) & M64 if check else 0), (what, r)
            assert t.check_failures == 0 and t.check_iters == (k * iters if check else 0), (what, r, t.check_iters)
            assert [l["peer"] for l in links] == list(peers), (what, r)
            assert t.nwg == max(l["nwg"] for l in links), (what, r)
            for j, l in enumerate(links):
                assert l["recv_done"] == iters, (what, r, l)
                assert l["recv_digest"] == ((iters * sums[j]) & M64 if check else 0), (what, r, l)
                assert l["check_failures"] == 0, (what, r, l)
                # (kernel entry is workgroup 0's stamp: a link's workgroups may all end within its tick)
                assert 0 <= l["device_s"] < 5.0, (what, r, l)
                if widths is not None:
                    assert l["nwg"] == widths, (what, r, l)

    def counters(self, r: int, p: int) -> dict:
        return self.c.link_counters(r, p)

    # ---- the links' counters (mpx_test_advance_link, mpx_link_counters) -----
    def advance(self, links, seq_by: int = 0, calls_by: int = 0) -> None:
        """each unordered link (r, p) given: both of its sides jump forward alike (between calls)"""
        for r, p in links:
            self.c.test_advance_link(r, p, seq_by, calls_by, 0)
            self.c.test_advance_link(p, r, seq_by, calls_by, 0)

    def advance_token(self, r: int, by: int) -> None:
        """the token is the rank's, not a link's: added once, through one of
        the rank's links, whose own counters stay where they are"""
        p = 0 if r else 1
        before = self.counters(r, p)
        self.c.test_advance_link(r, p, 0, 0, by)
        assert self.counters(r, p) == dict(before, token=before["token"] + by)

    def jump(self, link, next_push: int) -> None:
        """both ranks of the link: the next push is number `next_push` (hostpairs.jump)"""
        r, p = link
        c = [self.counters(r, p), self.counters(p, r)]
        last = c[0]["tx_seq"]
        assert all(x["tx_seq"] == last and x["rx_seq"] == last for x in c), c
        assert next_push - 1 > last
        self.advance([link], seq_by=next_push - 1 - last)
        for a, b in ((r, p), (p, r)):
            x = self.counters(a, b)
            assert x["tx_seq"] == x["rx_seq"] == next_push - 1, (a, b, x)

    def counted(self, peersets: dict, iters: int, call):
        """call(), and what it must have added to every link of the context,
        seen from both sides: iters pushes each way and one call on a link of
        the peer graph (no call number for iters = 0), nothing on any other
        link; one token for every rank that called"""
        pairs = [(r, p) for r in self.ranks for p in range(self.n) if p != r]
        before = {k: self.counters(*k) for k in pairs}
        out = call()
        for (r, p), b in before.items():
            a = self.counters(r, p)
            on = p in peersets.get(r, [])
            assert a["tx_seq"] == b["tx_seq"] + (iters if on else 0), (r, p, b, a)
            assert a["rx_seq"] == b["rx_seq"] + (iters if on else 0), (r, p, b, a)
            assert a["calls"] == b["calls"] + (1 if on and iters > 0 else 0), (r, p, b, a)
            assert a["token"] == b["token"] + (1 if r in peersets else 0), (r, p, b, a)
        return out

    def checked_call(self, peersets: dict, iters: int, check: bool, what, widths=None, **kw):
        """one fan call of every listed rank on a 0xEE-prefilled rx, nothing
        timed out or failed, then Fan.verify and Fan.counted"""
        def call():
            out, errs = self.run(peersets, iters, check=check, **kw)
            assert not errs, (what, errs)
            self.verify(peersets, out, iters, check, what, widths=widths)
            return out
        return self.counted(peersets, iters, call)
