"""Sequenced payloads on a loopback pair (-m gpu): helpers of
tests/test_gpu_seq.py and tests/seq_worker.py.

TEST INFRASTRUCTURE.  Every expectation comes from host bytes: the payload
rank s sends rank d in iteration i is oracle_py.fill(n, FILL_SPLITMIX,
mpx.pattern_key(seed, s, d, i)), its checksum oracle_py.checksum of those
bytes.  Nothing here asks the library what it would send.
"""
from __future__ import annotations

import functools
import threading

import mpx
import oracle_py as O
import payload
from hostpairs import M64, NONBLOCKING, UNIDIR
from payload import GUARD, assert_region

SEED = 0x5EC0DED5EED5EED5


@functools.lru_cache(maxsize=None)
def sent(seed: int, s: int, d: int, i: int, n: int) -> bytes:
    """P(seed, s, d, i, n): what rank s sends rank d in iteration i"""
    return O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(seed, s, d, i))


@functools.lru_cache(maxsize=None)
def csum(seed: int, s: int, d: int, i: int, n: int) -> int:
    return O.checksum(sent(seed, s, d, i, n))


def recv_len(P, mode, r, n):
    """bytes rank r receives per message: B, or unidir's 1-byte ack (group 1)"""
    return 1 if (mode == UNIDIR and r in P.group1) else n


def expectations(P, mode, r, n, iters, seed=SEED):
    """expect[]: the checksum of every payload rank r receives"""
    return [csum(seed, P.peer(r), r, i, recv_len(P, mode, r, n)) for i in range(iters)]


def counted(mode, iters):
    """the iterations whose receive the reference's loop completes"""
    return [i for i in range(iters) if mode != NONBLOCKING or i % 256 != 255]


def prefill(P, n):
    for r in P.ranks:      # (max: the 1-byte ack of a 0-byte unidir message has its guard too)
        P.c.fill(P.bufs[r][1], max(n, 1) + GUARD, mpx.FILL_BYTE, payload.GUARD_BYTE)


def run(P, mode, n, iters, seed=SEED, check=True, expect="host", seq_ranks=None, timeout_ms=10000, nwg=0, stream=False):
    """every rank's side on a thread of its own.  Ranks in seq_ranks (default:
    all) call xfer_seq, the others xfer (unchecked).  expect: "host" (the
    oracle's checksums), None (the library computes them) or {rank: list}.
    Returns ({rank: Timing}, {rank: MpxError})"""
    seq_ranks = list(P.ranks) if seq_ranks is None else list(seq_ranks)
    out, errs = {}, {}

    def side(r):
        args = (mode, P.group(r), r, P.peer(r), iters, P.bufs[r][0], P.bufs[r][1], n)
        try:
            if r in seq_ranks:
                e = None
                if check and expect == "host":
                    e = expectations(P, mode, r, n, iters, seed)
                elif check and isinstance(expect, dict):
                    e = expect[r]
                out[r] = P.c.xfer_seq(*args, seed, check_payload=check, expect=e, timeout_ms=timeout_ms, nwg=nwg,
                                      stream=stream)
            else:
                out[r] = P.c.xfer(*args, timeout_ms=timeout_ms, nwg=nwg, stream=stream)
        except mpx.MpxError as e:
            errs[r] = e

    th = [threading.Thread(target=side, args=(r,)) for r in P.ranks]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out, errs


def assert_rx(P, mode, n, last, what, seed=SEED, ranks=None):
    """rx of every rank holds the peer's payload of iteration `last`, guard and
    all; the whole of tx is what the host wrote there"""
    for r in (P.ranks if ranks is None else ranks):
        want = sent(seed, P.peer(r), r, last, recv_len(P, mode, r, n)) if last >= 0 else b""
        assert_region(P.c, P.bufs[r][1], 0, want, what=f"{what}: rx of rank {r}")
        payload.compare(P.c.read(P.bufs[r][0], P.caps[r]), P.host[r], 0, f"{what}: tx of rank {r} after the call")


def verified(P, mode, n, iters, what, seed=SEED, check=True, **kw):
    """one sequenced call on a 0xEE-prefilled rx, then everything a caller can
    see of it"""
    prefill(P, n)
    out, errs = run(P, mode, n, iters, seed=seed, check=check, **kw)
    assert not errs, (what, errs)
    done = counted(mode, iters)
    for r in P.ranks:
        t = out[r]
        m = recv_len(P, mode, r, n)
        assert t.recv_done == len(done), (what, r, t.recv_done)
        assert t.launches == 1 and t.check_failures == 0, (what, r, t.launches, t.check_failures)
        assert t.check_iters == (iters if check else 0), (what, r, t.check_iters)
        if check:
            assert t.recv_digest == sum(csum(seed, P.peer(r), r, i, m) for i in done) & M64, (what, r)
    assert_rx(P, mode, n, iters - 1, what, seed)
    return out
