"""The host link's full-duplex loop, for tests/test_gpu_hostlink_duplex.py.

TEST INFRASTRUCTURE.  Functions over a tests/hostlink.py LinkMap: both sides of
a full-duplex call (include/mpx_hostlink_duplex.h) on threads of their own,
joined with a time limit, and the verification of everything such a call
leaves behind against host bytes — the whole rx and tx of both ends, the
reference's receive count (iters - iters // 256), the oracle's checksums, and
every counter of every attached rank.
"""
from __future__ import annotations

import threading
import time

import mpx
import payload
from hostlink import JOIN_S, M64, LinkMap

NB_WINDOW = 256
MIN_CHUNK = 1024
DEFAULT_MAX_WG = 16        # kDefaultMaxWG (mpx_hostlink.h): the default width's cap, per direction


def counted_receives(iters: int) -> int:
    """the receives the reference's Waitall calls return (mpi_perf.c:108-111,
    122-123): slot 255 of each full window is never waited for"""
    return iters - iters // NB_WINDOW


def width(n: int, nwg: int = 0) -> int:
    """the per-direction width of a call: the asked one, else one workgroup per
    32 KiB up to 16; then at least 1 KiB per workgroup (hostlink_nwg)"""
    w = nwg if nwg > 0 else min(DEFAULT_MAX_WG, max(1, -(-n // (32 << 10))))
    return max(1, min(w, -(-n // MIN_CHUNK)))


def one_gpu(n: int, nlinks: int = 1) -> LinkMap:
    """GPU rank 0 with `nlinks` endpoints 1.., each a link of its own"""
    return LinkMap(n, 1 + nlinks, [0], range(1, 1 + nlinks), [(0, k) for k in range(1, 1 + nlinks)])


def run(h: LinkMap, links, n: int, iters: int, check: bool = False, nwg: int = 0, timeout_ms: int = 5000,
        stage: bool = True, delay=None, before=None):
    """Both sides of every link of `links` on threads of their own.  delay /
    before: by rank, as LinkMap.run.  h.entered[r] / h.returned[r]: monotonic
    stamps around that side's call.  Returns ({(link, rank): Timing},
    {(link, rank): MpxError}); raises if a side is still running after JOIN_S."""
    links = [tuple(l) for l in links]
    ends = [r for l in links for r in l]
    assert len(set(ends)) == len(ends) and all(l in h.links for l in links), links
    out, errs, h.seen, h.entered, h.returned = {}, {}, {}, {}, {}

    def side(link, r) -> None:
        g, e = link
        exp, _ = h.expect(r, e if r == g else g, n)
        kw = dict(check_payload=check, expect=exp, timeout_ms=timeout_ms, nwg=nwg)
        if delay and r in delay:
            time.sleep(delay[r])
        if before and r in before:
            h.seen[r] = before[r]()
        h.entered[r] = time.monotonic()
        try:
            if r == g:
                out[link, r] = h.c.xfer_hostlink_duplex(g, e, iters, *h.gpu[g], n, stage=stage, **kw)
            else:
                out[link, r] = h.c.host_xfer_duplex(e, g, iters, n, **kw)
        except mpx.MpxError as x:
            errs[link, r] = x
        h.returned[r] = time.monotonic()

    th = [threading.Thread(target=side, args=(l, r), daemon=True) for l in links for r in l]
    for t in th:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in th:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in th):
        raise AssertionError(f"a side of the full-duplex call is still running after {JOIN_S} s (lost hand-off)")
    return out, errs


def want_rx(h: LinkMap, peer: int, n: int, iters: int) -> bytes:
    """an rx after a call from the guard state: the peer's tx[0:n), then guards"""
    k = n if iters > 0 else 0
    return h.tx_bytes[peer][:k] + bytes([0xEE]) * (h.cap - k)


def verify(h: LinkMap, out, links, n: int, iters: int, check: bool, what="", nwg: int = 0) -> None:
    """every byte of both ends' rx and tx, and everything the call reported"""
    done = counted_receives(iters)
    for link in links:
        g, e = link
        for r, peer in ((g, e), (e, g)):
            t = out[tuple(link), r]
            w = f"{what}: link {link} rank {r} ({'GPU' if r == g else 'host'}) n {n} iters {iters} check {check}"
            payload.compare(h.rx(r), want_rx(h, peer, n, iters), 0, w + " rx")
            payload.compare(h.tx(r), h.tx_bytes[r], 0, w + " tx")
            assert t.recv_done == done, (w, t.recv_done, done)
            assert t.bytes == 2 * n * iters, w
            assert t.launches == (1 if r == g else 0), w
            assert t.protocol == mpx.PROTO_HOSTLINK_DUPLEX == 13, w
            assert t.nwg == width(n, nwg), (w, t.nwg)
            if check:
                exp, _ = h.expect(r, peer, n)
                assert t.check_failures == 0 and t.check_iters == iters, (w, t.check_failures, t.check_iters)
                assert t.recv_digest == (exp * done) & M64, w
            else:
                assert t.check_iters == 0 and t.recv_digest == 0 and t.check_failures == 0, w


def call(h: LinkMap, links, n: int, iters: int, check: bool = True, what="", **kw):
    """reset every rx, run, no error on any side, verify; every counter of
    every attached rank moved as for a non-blocking pair call (+iters, +iters,
    +1 on either end; the GPU rank's token + 1) and nothing else moved"""
    links = [tuple(l) for l in links]

    def go():
        h.reset_rx()
        out, errs = run(h, links, n, iters, check=check, **kw)
        assert not errs, (what, {k: str(x) for k, x in errs.items()})
        verify(h, out, links, n, iters, check, what, nwg=kw.get("nwg", 0))
        h.untouched([r for l in links for r in l], what)
        return out
    return h.counted(links, iters, go, what)
