"""A loopback pair whose every expectation comes from host bytes (-m gpu).

TEST INFRASTRUCTURE shared by tests/test_gpu_bytes.py and
tests/test_gpu_wrap.py: HostPairs keeps on the host what each rank's tx holds,
run_checked makes one checked call and compares everything a caller can see
with it, and advance / counters move and read the link's counters
(mpx_test_advance_link / mpx_link_counters).
"""
from __future__ import annotations

import mpx
import oracle_py as O
import payload
from pairs import Pairs
from payload import assert_region

M64 = 0xFFFFFFFFFFFFFFFF
PINGPONG, NONBLOCKING, UNIDIR = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING, mpx.MODE_UNIDIR
GUARD = payload.GUARD
P31, P32 = 1 << 31, 1 << 32
# non-blocking check mode with three receive slots per link (tests/test_gpu_wrap.py, tests/wrap_worker.py)
CREDIT_N = 4097
CREDIT_CAP = CREDIT_N + GUARD
CREDIT_RING = 2 * CREDIT_CAP      # MPX_CHECK_RING_BYTES: two slots of the attached length


class HostPairs(Pairs):
    """one loopback pair (the kernel engine unless told otherwise) with seeded
    tx, whose expected bytes and checksums all come from the host: host[r] =
    what rank r's tx holds.  ranks, nranks, caps: tests/pairs.py (ranks =
    [group 1's ranks..., their peers...]; the default is the pair (0, 1) of a
    two-rank context, rank 0 group 1); npairs > 1: that many pairs"""

    def __init__(self, cap, engine="kernel", ranks=None, nranks=None, caps=None, npairs=1):
        super().__init__(engine, npairs, cap, fill="seeded", ranks=ranks, nranks=nranks, caps=caps)
        self.host = {r: O.fill(self.caps[r], mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 0, 0))
                     for r in self.ranks}

    def set_tx(self, data: bytes):
        """every rank's tx[0 : len(data)) = data (between calls)"""
        for r in self.ranks:
            payload.write(self.c, self.bufs[r][0], data)
            self.host[r] = data + self.host[r][len(data):]

    def expect(self, r, n):
        """what check mode is told to expect: host checksums of the peer's tx"""
        h = self.host[self.peer(r)]
        return O.checksum(h[:n]), O.checksum(h[:1])

    def advance(self, seq_by=0, calls_by=0, token_by=0):
        """both ranks of every link jump forward alike (between calls)"""
        for r in self.ranks:
            self.c.test_advance_link(r, self.peer(r), seq_by, calls_by, token_by)

    def counters(self, r):
        """rank r's side of the link: tx_seq, rx_seq, calls, token"""
        return self.c.link_counters(r, self.peer(r))


def received(mode, r, n, group1=(0,)):
    """bytes rank r receives per message: B, or unidir's 1-byte ack (group 1,
    mpi_perf.c:137,142; rank 0 in the default pair)"""
    return 1 if (mode == UNIDIR and r in group1) else n


def run_checked(P, mode, n, iters, what, **kw):
    """one checked call on a 0xEE-prefilled rx, then everything a caller can
    see: no error, every payload checked, the reference's receive count, the
    host-computed digest, rx byte for byte with its guard, tx untouched
    (check=False: an unchecked call, which checks and digests nothing)"""
    chk = kw.get("check", True)
    for r in P.ranks:      # (max: the 1-byte ack of a 0-byte unidir message has its guard too)
        P.c.fill(P.bufs[r][1], max(n, 1) + GUARD, mpx.FILL_BYTE, payload.GUARD_BYTE)
    out, errs = P.run(mode, n, iters, **kw)
    assert not errs, (what, errs)
    done = O.lib().oracle_nb_waited(iters) if mode == NONBLOCKING else iters
    for r in P.ranks:
        t = out[r]
        expected = P.host[P.peer(r)][:received(mode, r, n, P.group1)]
        assert t.check_failures == 0 and t.check_iters == (iters if chk else 0), (what, r, t.check_iters)
        assert t.recv_done == done, (what, r, t.recv_done)
        assert not chk or t.recv_digest == (done * O.checksum(expected)) & M64, (what, r)
        assert_region(P.c, P.bufs[r][1], 0, expected, what=f"{what}: rx of rank {r}")
        # (the whole of tx, not only the n bytes sent: a push that landed in it lands anywhere)
        payload.compare(P.c.read(P.bufs[r][0], P.caps[r]), P.host[r], 0, f"{what}: tx of rank {r} after the call")
    return out


def jump(P, next_push):
    """both ranks of the link: the next push is number `next_push`"""
    c = [P.counters(r) for r in P.ranks]
    last = c[0]["tx_seq"]
    assert all(x["tx_seq"] == last and x["rx_seq"] == last for x in c), c
    assert next_push - 1 > last
    P.advance(seq_by=next_push - 1 - last)
    for r in P.ranks:
        assert P.counters(r)["tx_seq"] == P.counters(r)["rx_seq"] == next_push - 1


def counted(P, iters, call, what):
    """call(), and what it must have added to both ranks' counters: iters
    pushes each way, one call on the link (none for iters = 0), one token on
    the kernel engine"""
    before = {r: P.counters(r) for r in P.ranks}
    out = call()
    for r in P.ranks:
        b, a = before[r], P.counters(r)
        assert a["tx_seq"] == b["tx_seq"] + iters and a["rx_seq"] == b["rx_seq"] + iters, (what, r, b, a)
        assert a["calls"] == b["calls"] + (1 if iters > 0 else 0), (what, r, b, a)
        assert a["token"] == b["token"] + (1 if P.c.engine == mpx.ENGINE_KERNEL else 0), (what, r, b, a)
    return out


def checked(P, mode, n, iters, what, **kw):
    return counted(P, iters, lambda: run_checked(P, mode, n, iters, what, **kw), what)
