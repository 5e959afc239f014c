"""Sequenced fan payloads (mpx_xfer_fan_seq, include/mpx_fan_seq.h) on loopback
ranks: helpers of tests/test_gpu_fan_seq.py, tests/fan_seq_worker.py and the
CPU tests of tests/test_fan_seq_abi.py.

TEST INFRASTRUCTURE.  Every expectation comes from host bytes: the block rank
s pushes to rank d in iteration i is oracle_py.fill(n, FILL_SPLITMIX,
mpx.pattern_key(seed, s, d, i)), its checksum oracle_py.checksum of those
bytes.  Nothing here asks the library what it would send.  tests/fan.py's Fan
gives the ranks, their tx images (which a sequenced call must leave alone and
must not send) and the link counters.
"""
from __future__ import annotations

import functools
import threading

import mpx
import oracle_py as O
import payload
from fan import M64, Fan, round16

SEED = 0xFA25EC0DED5EED51
PROTO = {False: 9, True: 10}      # mpx_timing.protocol: bulk fan, lock-step LL fan


@functools.lru_cache(maxsize=256)
def sent(seed: int, s: int, d: int, i: int, n: int) -> bytes:
    """P(seed, s, d, i, n): the block rank s pushes to rank d in iteration i"""
    return O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(seed, s, d, i))


@functools.lru_cache(maxsize=None)
def csum(seed: int, s: int, d: int, i: int, n: int) -> int:
    """the checksum of P(seed, s, d, i, n); the bytes of a large block are not
    kept (a 33-iteration call on 12 links of 256 KiB would hold 100 MB)"""
    if n > 65536:
        return O.checksum(O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(seed, s, d, i)))
    return O.checksum(sent(seed, s, d, i, n))


def expectations(r: int, peers, n: int, iters: int, seed: int = SEED) -> list:
    """expect[k * iters + i]: the checksum of payload i of link k, in the caller's order of peers"""
    return [csum(seed, p, r, i, n) for p in peers for i in range(iters)]


def expected_rx(cap: int, stride: int, n: int, r: int, peers, last: int, seed: int = SEED) -> bytes:
    """the whole of rank r's rx after a completed call whose last iteration
    was `last` (-1: nothing moved): block p = P(seed, p, r, last, n) for every
    peer, 0xEE everywhere else (the gaps, r's own block, the blocks of ranks
    outside the peer set, the guard)"""
    want = bytearray([payload.GUARD_BYTE]) * cap
    if last >= 0:
        for p in peers:
            want[p * stride:p * stride + n] = sent(seed, p, r, last, n)
    return bytes(want)


def check_rx(got: bytes, cap: int, stride: int, n: int, r: int, peers, last: int, what, seed: int = SEED) -> None:
    """got is expected_rx(...), or an AssertionError that names the range: the
    block of the rank it should hold, or the untouched bytes that follow it"""
    want = expected_rx(cap, stride, n, r, peers, last, seed)
    assert len(got) == cap, (what, len(got), cap)
    nblocks = cap // stride
    for j in range(nblocks):
        lo = j * stride
        kind = f"block of peer {j}, iteration {last}" if j in peers and last >= 0 else f"untouched block {j}"
        payload.compare(got[lo:lo + n], want[lo:lo + n], lo, f"{what}: rx of rank {r}, {kind} [{lo}, {lo + n})")
        payload.compare(got[lo + n:lo + stride], want[lo + n:lo + stride], lo + n,
                        f"{what}: rx of rank {r}, gap after block {j} [{lo + n}, {lo + stride})")
    payload.compare(got[nblocks * stride:], want[nblocks * stride:], nblocks * stride,
                    f"{what}: rx of rank {r}, guard [{nblocks * stride}, {cap})")


def mesh(nranks: int, n: int, stride: int = 0, ranks=None) -> Fan:
    """a Fan of `nranks` (attached: ranks, default all) laid out for blocks of n
    bytes; the default stride leaves a gap after every block"""
    stride = stride or round16(n) + 16
    F = Fan(nranks, nranks * stride + payload.GUARD, ranks=ranks)
    F.layout(n, stride)
    return F


def run(F: Fan, peersets: dict, iters: int, seed: int = SEED, check=True, expect="host", seq_ranks=None, ll=False,
        timeout_ms=5000, prefill=True, **kw):
    """every listed rank's call on a thread of its own.  Ranks in seq_ranks
    (default: all) call xfer_fan_seq, the others an ordinary unchecked fan
    call.  expect: "host" (the oracle's checksums), None (the library
    computes them) or {rank: list}.  -> ({rank: (Timing, links)}, {rank: MpxError})"""
    assert timeout_ms <= 5000
    seq_ranks = list(peersets) if seq_ranks is None else list(seq_ranks)
    if prefill:
        F.prefill()
    out, errs = {}, {}

    def side(r):
        tx, rx = F.bufs[r]
        try:
            if r in seq_ranks:
                e = None
                if check and expect == "host":
                    e = expectations(r, peersets[r], F.block_len, iters, seed)
                elif check and isinstance(expect, dict):
                    e = expect[r]
                out[r] = F.c.xfer_fan_seq(r, peersets[r], iters, tx, rx, F.block_len, F.stride, seed, check_payload=check,
                                          expect=e, timeout_ms=timeout_ms, ll=ll, **kw)
            else:
                out[r] = F.c.fan(r, peersets[r], iters, tx, rx, F.block_len, F.stride, timeout_ms=timeout_ms, ll=ll, **kw)
        except mpx.MpxError as e:
            errs[r] = e

    th = [threading.Thread(target=side, args=(r,)) for r in peersets]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out, errs


def verify_bytes(F: Fan, peersets: dict, last: int, what, seed: int = SEED, ranks=None) -> None:
    """rx whole and tx whole of every attached rank, read back"""
    for r in (F.ranks if ranks is None else ranks):
        check_rx(F.c.read(F.bufs[r][1], F.caps[r]), F.caps[r], F.stride, F.block_len, r, peersets.get(r, []), last, what,
                 seed)
        payload.compare(F.c.read(F.bufs[r][0], F.caps[r]), F.host[r], 0, f"{what}: tx of rank {r}")


def verify(F: Fan, peersets: dict, out: dict, iters: int, check: bool, what, seed: int = SEED, ll=False, widths=None):
    """the bytes, and everything a completed call reports, per link and in total"""
    verify_bytes(F, peersets, iters - 1, what, seed)
    n = F.block_len
    for r, peers in peersets.items():
        t, links = out[r]
        k = len(peers)
        assert t.protocol == PROTO[ll] and t.launches == 1, (what, r, t.protocol, t.launches)
        assert t.bytes == 2 * n * iters * k and t.recv_done == k * iters, (what, r, t.bytes, t.recv_done)
        sums = [sum(csum(seed, p, r, i, n) for i in range(iters)) & M64 if check else 0 for p in peers]
        assert t.recv_digest == sum(sums) & M64, (what, r)
        assert t.check_failures == 0 and t.check_iters == (k * iters if check else 0), (what, r, t.check_iters)
        assert [l["peer"] for l in links] == list(peers), (what, r)
        assert t.nwg == max(l["nwg"] for l in links), (what, r)
        for j, l in enumerate(links):
            assert l["recv_done"] == iters and l["check_failures"] == 0, (what, r, l)
            assert l["recv_digest"] == sums[j], (what, r, l)
            assert 0 <= l["device_s"] < 5.0, (what, r, l)
            if ll:
                assert l["nwg"] == 1, (what, r, l)
            elif widths is not None:
                assert l["nwg"] == widths, (what, r, l)


def verified(F: Fan, peersets: dict, iters: int, what, seed: int = SEED, check=True, ll=False, widths=None, **kw):
    """one sequenced call of every listed rank on a 0xEE-prefilled rx: nothing
    failed, the bytes, the reports and the link counters (Fan.counted)"""
    def call():
        out, errs = run(F, peersets, iters, seed=seed, check=check, ll=ll, **kw)
        assert not errs, (what, errs)
        verify(F, peersets, out, iters, check, what, seed=seed, ll=ll, widths=widths)
        return out
    return F.counted(peersets, iters, call)
