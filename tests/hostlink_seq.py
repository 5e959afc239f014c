"""Sequenced payloads on the host link (mpx_xfer_hostlink_seq /
mpx_host_xfer_seq, include/mpx_hostlink_seq.h): helpers of
tests/test_gpu_hostlink_seq.py and tests/hostlink_seq_worker.py.

TEST INFRASTRUCTURE.  A LinkMap (tests/hostlink.py) supplies the ranks, the
buffers and the counters.  Every expectation comes from host bytes: the
payload rank s sends rank d in iteration i is seq.sent(seed, s, d, i, n) =
oracle_py.fill under mpx.pattern_key, its checksum oracle_py.checksum of those
bytes.  Nothing here asks the library what it would send.  Before every call
both rx hold 0xEE from end to end (the guards are the n + SLACK bytes past the
message) and the endpoint's tx is drawn anew from a seed of LinkMap's own,
which is none of the payloads; the GPU rank's tx keeps the bytes it was seeded
with, which every call must leave as they were.
"""
from __future__ import annotations

import threading
import time

import mpx
import payload
from hostlink import GUARD_BYTE, JOIN_S, M64, LinkMap
from seq import SEED, csum, sent

PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
BIG = (256 << 10) + 21
LINK = (0, 1)

_reseeds = [0]


def one(n: int) -> LinkMap:
    """GPU rank 0 and endpoint 1, built for messages of n bytes"""
    return LinkMap(n, 2, [0], [1], [LINK])


def lens(mode: int, group: int, n: int):
    """(bytes sent, bytes received) per message by a side of that group"""
    return (1 if (mode == UNI and group == 0) else n), (1 if (mode == UNI and group == 1) else n)


def expectations(src: int, dst: int, m: int, iters: int, seed: int = SEED):
    """expect[]: the checksum of every payload dst receives from src"""
    return [csum(seed, src, dst, i, m) for i in range(iters)]


def prepare(h: LinkMap, link=LINK) -> None:
    """every rx back to 0xEE and the endpoint's tx drawn anew"""
    h.reset_rx()
    _reseeds[0] += 1
    h.set_tx(link[1], 0x5E0000 + _reseeds[0])


def run(h: LinkMap, link, mode: int, gpu_group: int, n: int, iters: int, seed: int = SEED, check: bool = True,
        expect="host", seq_sides=("gpu", "host"), nwg: int = 0, timeout_ms: int = 5000, flags: int = 0):
    """Both sides of the link on threads of their own.  A side named in
    seq_sides makes the sequenced call, the other the ordinary one
    (unchecked).  expect: "host" (the oracle's checksums) or None (the library
    computes them).  Returns ({rank: Timing}, {rank: MpxError}); raises if a
    side is still running after JOIN_S."""
    g, e = link
    out, errs = {}, {}

    def side(r: int) -> None:
        gpu_side = r == g
        group = gpu_group if gpu_side else 1 - gpu_group
        peer = e if gpu_side else g
        try:
            if ("gpu" if gpu_side else "host") in seq_sides:
                want = expectations(peer, r, lens(mode, group, n)[1], iters, seed) if (check and expect == "host") else None
                kw = dict(check_payload=check, expect=want, timeout_ms=timeout_ms, nwg=nwg, flags=flags)
                if gpu_side:
                    out[r] = h.c.xfer_hostlink_seq(mode, group, g, e, iters, *h.gpu[g], n, seed, **kw)
                else:
                    out[r] = h.c.host_xfer_seq(mode, group, e, g, iters, n, seed, **kw)
            elif gpu_side:
                out[r] = h.c.xfer_hostlink(mode, group, g, e, iters, *h.gpu[g], n, timeout_ms=timeout_ms, nwg=nwg)
            else:
                out[r] = h.c.host_xfer(mode, group, e, g, iters, n, timeout_ms=timeout_ms, nwg=nwg)
        except mpx.MpxError as x:
            errs[r] = x

    th = [threading.Thread(target=side, args=(r,), daemon=True) for r in link]
    for t in th:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in th:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in th):
        raise AssertionError(f"a side of the host link is still running after {JOIN_S} s (lost hand-off)")
    return out, errs


def want_rx(h: LinkMap, src: int, dst: int, m: int, last: int, seed: int = SEED) -> bytes:
    """dst's whole rx after a call from the guard state: src's payload of
    iteration `last` (none: last < 0), then guards"""
    got = sent(seed, src, dst, last, m) if last >= 0 else b""
    return got + bytes([GUARD_BYTE]) * (h.cap - len(got))


def want_host_tx(h: LinkMap, link, mode: int, gpu_group: int, n: int, last: int, seed: int = SEED, ll_max=None) -> bytes:
    """the endpoint's whole tx after a sequenced call: its payload of iteration
    `last` over [0, send_len) where its sends were bulk, else untouched"""
    g, e = link
    ll_max = mpx.hostlink_ll_max() if ll_max is None else ll_max
    m = lens(mode, 1 - gpu_group, n)[0]
    was = h.tx_bytes[e]
    if last < 0 or m <= ll_max:
        return was
    return sent(seed, e, g, last, m) + was[m:]


def verify(h: LinkMap, out, link, mode: int, gpu_group: int, n: int, iters: int, seed: int = SEED, check: bool = True,
           what="", ll_max=None) -> None:
    """every byte of both ends' rx and tx, and everything the call reported"""
    g, e = link
    ll_max = mpx.hostlink_ll_max() if ll_max is None else ll_max
    for r, peer, group in ((g, e, gpu_group), (e, g, 1 - gpu_group)):
        t = out[r]
        m = lens(mode, group, n)[1]
        w = f"{what}: rank {r} ({'GPU' if r == g else 'host'}, group {group}) mode {mode} n {n} iters {iters}"
        payload.compare(h.rx(r), want_rx(h, peer, r, m, iters - 1, seed), 0, w + " rx")
        want_tx = h.tx_bytes[g] if r == g else want_host_tx(h, link, mode, gpu_group, n, iters - 1, seed, ll_max)
        payload.compare(h.tx(r), want_tx, 0, w + " tx")
        assert t.recv_done == iters, (w, t.recv_done)
        assert t.bytes == n * iters * (1 if mode == UNI else 2), w
        assert t.launches == (1 if r == g else 0), w
        assert t.protocol == (mpx.PROTO_HOSTLINK_LL if n <= ll_max else mpx.PROTO_HOSTLINK_BULK), (w, t.protocol)
        if check:
            assert t.check_failures == 0 and t.check_iters == iters, (w, t.check_failures, t.check_iters)
            assert t.recv_digest == sum(expectations(peer, r, m, iters, seed)) & M64, w
        else:
            assert t.check_iters == 0 and t.recv_digest == 0 and t.check_failures == 0, w


def call(h: LinkMap, mode: int, gpu_group: int, n: int, iters: int, seed: int = SEED, check: bool = True, expect="host",
         what="", link=LINK, ll_max=None, **kw):
    """prepare, one sequenced call on both ends, no error, verify; every
    counter of both ends moved as an ordinary host-link call moves them"""
    def go():
        prepare(h, link)
        out, errs = run(h, link, mode, gpu_group, n, iters, seed=seed, check=check, expect=expect, **kw)
        assert not errs, (what, {k: str(x) for k, x in errs.items()})
        verify(h, out, link, mode, gpu_group, n, iters, seed, check, what, ll_max)
        return out
    return h.counted([link], iters, go, what)


def record(out, errs, r):
    """what a worker reports of one side of a call"""
    t = errs[r].timing if r in errs else out[r]
    return {"status": errs[r].status if r in errs else mpx.OK, "check_failures": t.check_failures,
            "check_iters": t.check_iters, "recv_done": t.recv_done}
