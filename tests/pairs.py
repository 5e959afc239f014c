"""Pairs of ranks of one process, for the -m gpu tests.

`npairs` pairs in the reference's -p layout (mpi_perf.c:437-450 with ppn =
npairs): ranks [0, np) are group 1, ranks [np, 2np) group 0, rank k is paired
with np + k.  Each rank runs its side of the loop on a host thread of its own,
like one MPI rank each.

`devs` maps rank -> GPU.  The default puts every rank on GPU 0 (loopback
pairs: the kernel, mailbox protocol and sequence bookkeeping of the cross-GPU
path, with the peer's HBM being local HBM); `cross_gpu_devs()` puts every
rank on a GPU of its own, so each pair moves its bytes over xGMI.

`ranks` gives the 2 * npairs ranks numbers of their own in a context of
`nranks` ranks (default: the largest number + 1), of which only these are
attached: ranks[k] is group 1 and paired with ranks[np + k].  `caps` (rank ->
bytes) attaches single ranks with another length than `cap`.  The defaults are
the layout above.
"""
from __future__ import annotations

import os
import threading

import mpx

def rehearsing() -> bool:
    """MPX_MULTI_REHEARSE=1: run the multi-GPU tests' code on one GPU (every
    rank on GPU 0) to shake out the tests themselves.  Read per call: on a
    one-GPU box tests/test_gpu_multi.py sets it per test (a fixture), so the
    driver's `pytest -m gpu` runs that rehearsal; subprocess workers inherit
    it through the environment."""
    return bool(os.environ.get("MPX_MULTI_REHEARSE"))


def cross_gpu_devs(nranks: int) -> list[int] | None:
    """rank r on GPU r, or None when fewer than nranks GPUs are visible
    (rehearsal: every rank on GPU 0)"""
    if rehearsing():
        return [0] * nranks
    return list(range(nranks)) if mpx.device_count() >= nranks else None


class Pairs:
    def __init__(self, engine, npairs, cap, fill="compat", devs=None, ranks=None, nranks=None, caps=None):
        self.np = npairs
        self.ranks = list(range(2 * npairs)) if ranks is None else list(ranks)
        assert len(self.ranks) == 2 * npairs == len(set(self.ranks)), self.ranks
        self.group1 = self.ranks[:npairs]
        self._peer = {}
        for k in range(npairs):
            a, b = self.ranks[k], self.ranks[npairs + k]
            self._peer[a], self._peer[b] = b, a
        self.nranks = max(self.ranks) + 1 if nranks is None else nranks
        self.c = mpx.Context(self.nranks, engine)
        self.cap = cap
        self.caps = {r: (caps or {}).get(r, cap) for r in self.ranks}
        devs = list(devs) if devs is not None else [0] * (2 * npairs)
        assert len(devs) == 2 * npairs
        self.devs = devs
        self.bufs = {}      # rank -> (tx, rx)
        for r, d in zip(self.ranks, devs):
            n = self.caps[r]
            tx, rx = self.c.alloc(d, n), self.c.alloc(d, n)
            if fill == "compat":   # mpi_perf.c:244-251: group 0 'a', group 1 'b'
                self.c.fill(tx, n, mpx.FILL_BYTE, ord("b") if r in self.group1 else ord("a"))
            else:
                self.c.fill(tx, n, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 0, 0))
            self.c.fill(rx, n, mpx.FILL_BYTE, 0)
            self.c.attach(r, d, tx, rx, n)
            self.bufs[r] = (tx, rx)
        if self.c.engine == mpx.ENGINE_RCCL:
            self.c.rccl_init_all()

    def peer(self, r):
        return self._peer[r]

    def group(self, r):
        return 1 if r in self.group1 else 0

    def expect(self, r, n):
        tx = self.bufs[self.peer(r)][0]
        return self.c.checksum(tx, n), self.c.checksum(tx, 1)

    def run(self, mode, n, iters, check=True, timeout_ms=10000, ranks=None, nwg=0, stream=False, pull=False,
            armed=False, stage=True):
        """every rank's side on a thread of its own; armed: each side arms
        its call (mpx_xfer_arm), all sides meet at a barrier (the hosts'
        mpi_perf.c:499), then start it; stage=False: MPX_XFER_NOSTAGE"""
        ranks = list(self.ranks) if ranks is None else ranks
        exp = {r: self.expect(r, n) for r in ranks}
        out, errs = {}, {}
        bar = threading.Barrier(len(ranks))

        def side(r):
            kw = dict(check_payload=check, expect=exp[r][0], expect_ack=exp[r][1], timeout_ms=timeout_ms, nwg=nwg,
                      stream=stream, pull=pull, stage=stage)
            args = (mode, self.group(r), r, self.peer(r), iters, self.bufs[r][0], self.bufs[r][1], n)
            try:
                if armed:
                    self.c.arm(*args, **kw)
                    bar.wait()
                out[r] = self.c.xfer(*args, **kw)
            except mpx.MpxError as e:
                errs[r] = e
                if armed:
                    bar.abort()

        th = [threading.Thread(target=side, args=(r,)) for r in ranks]
        for t in th:
            t.start()
        for t in th:
            t.join()
        return out, errs

    def close(self):
        self.c.close()
