"""Loopback ranks for the fan-exchange tests (tests/test_gpu_fan.py, -m gpu).

TEST INFRASTRUCTURE: plain classes and functions, no fixtures.  N ranks on
GPU 0, one host thread per rank and call, every expectation from host bytes:
host[r] is what rank r's tx holds (block d, for rank d, seeded with the key of
(r, d); the bytes between blocks seeded too, so a push that read the wrong
place shows), rx is 0xEE before every call, and after it the WHOLE of rx and
of tx is read back and compared byte for byte.
"""
from __future__ import annotations

import threading

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


class Fan:
    def __init__(self, nranks: int, cap: int, engine="kernel"):
        self.n = nranks
        self.cap = cap
        self.c = mpx.Context(nranks, engine)
        self.bufs = []
        self.host = [b""] * nranks
        self.block_len = self.stride = 0
        for r in range(nranks):
            tx, rx = self.c.alloc(0, cap), self.c.alloc(0, cap)
            self.c.attach(r, 0, tx, rx, cap)
            self.bufs.append((tx, rx))

    def close(self):
        self.c.close()

    def layout(self, block_len: int, stride: int) -> None:
        """every rank's tx, written from the host for this block layout"""
        assert self.n * stride <= self.cap and block_len <= stride
        self.block_len, self.stride = block_len, stride
        for r in range(self.n):
            h = bytearray(O.fill(self.cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 63, 1)))
            for d in range(self.n):
                h[d * stride:d * stride + block_len] = O.fill(block_len, mpx.FILL_SPLITMIX,
                                                              mpx.pattern_key(mpx.PATTERN_SEED, r, d, 7))
            self.host[r] = bytes(h)
            payload.write(self.c, self.bufs[r][0], self.host[r])

    def block(self, src: int, dst: int) -> bytes:
        """what src sends dst"""
        return self.host[src][dst * self.stride:dst * self.stride + self.block_len]

    def prefill(self) -> None:
        for r in range(self.n):
            self.c.fill(self.bufs[r][1], self.cap, mpx.FILL_BYTE, payload.GUARD_BYTE)

    def run(self, peersets: dict, iters: int, check=True, timeout_ms=5000, prefill=True, **kw):
        """peersets: rank -> its peers, in the order it lists them; every
        listed rank calls on a thread of its own"""
        if prefill:
            self.prefill()
        out, errs = {}, {}

        def side(r):
            exp = [O.checksum(self.block(p, r)) for p in peersets[r]]
            try:
                out[r] = self.c.fan(r, peersets[r], iters, self.bufs[r][0], self.bufs[r][1], self.block_len, self.stride,
                                    check_payload=check, expect=exp, timeout_ms=timeout_ms, **kw)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,)) for r in peersets]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return out, errs

    def expected_rx(self, r: int, peers, moved=True) -> bytes:
        want = bytearray([payload.GUARD_BYTE]) * self.cap
        if moved:
            for p in peers:
                want[p * self.stride:p * self.stride + self.block_len] = self.block(p, r)
        return bytes(want)

    def verify_bytes(self, peersets: dict, what, moved=True) -> None:
        """rx whole (the peers' blocks, 0xEE everywhere else: the gaps, the
        rank's own block, the blocks of ranks outside the set) and tx whole"""
        for r in range(self.n):
            peers = peersets.get(r, [])
            payload.compare(self.c.read(self.bufs[r][1], self.cap), self.expected_rx(r, peers, moved), 0,
                            f"{what}: rx of rank {r}")
            payload.compare(self.c.read(self.bufs[r][0], self.cap), self.host[r], 0, f"{what}: tx of rank {r}")

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
