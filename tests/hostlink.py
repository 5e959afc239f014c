"""Host links of one process, for tests/test_gpu_hostlink.py.

TEST INFRASTRUCTURE.  `npairs` GPU ranks [0, np) on GPU 0, each paired with a
host endpoint of its own, np + k (include/mpx_hostlink.h).  Every buffer is
attached `slack` bytes longer than the message size the link is built for; tx
holds host bytes this module seeded (oracle_py.fill, one key per rank), so
every expectation is built on the host from those bytes.  Each side of a call
runs on a thread of its own, like tests/pairs.py; the threads are joined with
a time limit, and a side that is still running then fails the test instead of
blocking it.
"""
from __future__ import annotations

import ctypes as C
import threading
import time

import mpx
import oracle_py
import payload

SLACK = 4096
GUARD_BYTE = 0xEE
JOIN_S = 30.0


class HostLinks:
    def __init__(self, n: int, npairs: int = 1, slack: int = SLACK):
        self.np = npairs
        self.cap = n + slack
        self.c = mpx.Context(2 * npairs, "kernel")
        self.tx_bytes = {}     # rank -> the host bytes its tx holds
        self.gpu = {}          # GPU rank -> (tx, rx) device buffers
        self.host = {}         # host endpoint -> (tx, rx) ctypes arrays over its pinned memory
        for r in range(2 * npairs):
            data = oracle_py.fill(self.cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 0, 0))
            self.tx_bytes[r] = data
            if r < npairs:
                tx, rx = self.c.alloc(0, self.cap), self.c.alloc(0, self.cap)
                payload.write(self.c, tx, data)
                self.c.attach(r, 0, tx, rx, self.cap)
                self.gpu[r] = (tx, rx)
            else:
                self.c.host_attach(r, self.cap)
                tx, rx = self.c.host_buffers(r)
                C.memmove(tx, data, self.cap)
                self.host[r] = (tx, rx)
        self.reset_rx()

    def peer(self, r: int) -> int:
        return r + self.np if r < self.np else r - self.np

    def reset_rx(self) -> None:
        """every rx back to the guard byte (between calls only)"""
        for tx, rx in self.gpu.values():
            self.c.fill(rx, self.cap, mpx.FILL_BYTE, GUARD_BYTE)
        for tx, rx in self.host.values():
            C.memset(rx, GUARD_BYTE, self.cap)

    def rx(self, r: int) -> bytes:
        """all of rank r's rx, as host bytes"""
        if r < self.np:
            return self.c.read(self.gpu[r][1], self.cap)
        return bytes(self.host[r][1])

    def expect(self, r: int, n: int):
        """(checksum of the peer's tx[0:n), checksum of its tx[0:1)): host bytes, the oracle's checksum"""
        data = self.tx_bytes[self.peer(r)]
        return oracle_py.checksum(data[:n]), oracle_py.checksum(data[:1])

    def want_rx(self, r: int, mode: int, group: int, n: int, iters: int) -> bytes:
        """what rank r's rx holds after a call from the guard state: the
        received range (the unidir sender's: the one ack byte), then guards"""
        got = 0 if iters == 0 else (1 if (mode == mpx.MODE_UNIDIR and group == 1) else n)
        return self.tx_bytes[self.peer(r)][:got] + bytes([GUARD_BYTE]) * (self.cap - got)

    def run(self, mode: int, gpu_group: int, n: int, iters: int, check: bool = False, nwg: int = 0,
            timeout_ms: int = 5000, pairs=None, delay=None, before=None):
        """Every side of the pairs `pairs` (default: all) on a thread of its
        own.  delay: {rank: seconds} a side sleeps before it enters; before:
        {rank: callable} run on that side's thread right before it enters,
        its result kept in self.seen[rank].  Returns (timings, errors) by
        rank; raises if a side is still running after JOIN_S."""
        pairs = list(range(self.np)) if pairs is None else list(pairs)
        out, errs, self.seen = {}, {}, {}

        def side(r: int) -> None:
            gpu_side = r < self.np
            group = gpu_group if gpu_side else 1 - gpu_group
            exp, ack = self.expect(r, n)
            kw = dict(check_payload=check, expect=exp, expect_ack=ack, timeout_ms=timeout_ms, nwg=nwg)
            if delay and r in delay:
                time.sleep(delay[r])
            if before and r in before:
                self.seen[r] = before[r]()
            try:
                if gpu_side:
                    out[r] = self.c.xfer_hostlink(mode, group, r, self.peer(r), iters, *self.gpu[r], n, **kw)
                else:
                    out[r] = self.c.host_xfer(mode, group, r, self.peer(r), iters, n, **kw)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,), daemon=True) for k in pairs for r in (k, k + self.np)]
        for t in th:
            t.start()
        deadline = time.monotonic() + JOIN_S
        for t in th:
            t.join(max(0.0, deadline - time.monotonic()))
        if any(t.is_alive() for t in th):
            raise AssertionError(f"a side of the host link is still running after {JOIN_S} s (lost hand-off)")
        return out, errs

    def close(self) -> None:
        self.c.close()
