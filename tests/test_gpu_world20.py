"""World 20 on one GPU: scripts/run-hbv3.sh's shape (2 hosts x 10 flows, rank
k paired with 10 + k) as twenty loopback ranks of one process, one host
thread per rank.

Twenty rank streams are twenty dedicated hardware queues in one process, and
the checked unidir call keeps 20 kernels x bulk_nwg(456131) = 28 workgroups
resident together.  Every expectation comes from host bytes
(tests/hostpairs.py), and mpx_link_counters of every (rank, peer) of the
twenty is read before and after each call: only the ten real links move.
The golden runs at ppn 10 (tests/golden/ref_runs.json) are run by the
fixture-driven tests of test_gpu_engine.py, test_gpu_pull.py and
test_gpu_host.py.
"""
import pytest

from fan import pair_nwg
from hostpairs import GUARD, NONBLOCKING, PINGPONG, UNIDIR, HostPairs, run_checked

pytestmark = pytest.mark.gpu

NP = 10
B = 456131      # scripts/run-hbv3.sh: -b 456131


def all_counters(P):
    return {(r, p): P.c.link_counters(r, p) for r in P.ranks for p in P.ranks if p != r}


def counted_all(P, iters, call, what):
    """call(), and what it added to the counters of all 20 x 19 (rank, peer)
    rows: iters pushes each way and one call on the ten real links, nothing
    on any other row; one token for every rank"""
    before = all_counters(P)
    out = call()
    for (r, p), b in before.items():
        on = P.peer(r) == p
        want = dict(tx_seq=b["tx_seq"] + (iters if on else 0), rx_seq=b["rx_seq"] + (iters if on else 0),
                    calls=b["calls"] + (1 if on else 0), token=b["token"] + 1)
        assert P.c.link_counters(r, p) == want, (what, r, p, b, P.c.link_counters(r, p))
    return out


def test_ten_pairs_every_loop_host_bytes_and_all_380_counter_rows():
    P = HostPairs(B + GUARD, npairs=NP)
    try:
        assert P.ranks == list(range(20)) and all(P.peer(k) == NP + k and P.group(k) == 1 for k in range(NP))
        assert pair_nwg(B) == 28
        calls = [(UNIDIR, B, 10, True, 1),           # run-hbv3's own call, every payload checked
                 (UNIDIR, B, 10, False, 1),          # and as the benchmark runs it
                 (PINGPONG, 8, 40, True, 0),         # LL: ten pairs' landing-zone rows at slots 0-19
                 (NONBLOCKING, 4097, 300, True, 1)]  # 20 receive rings
        for mode, n, iters, check, proto in calls:
            what = ("world 20", mode, n, iters, check)
            out = counted_all(P, iters, lambda: run_checked(P, mode, n, iters, what, check=check, timeout_ms=5000),
                              what)
            for r in P.ranks:
                assert out[r].protocol == proto, (what, r, out[r].protocol)
                assert out[r].bytes == n * iters * (1 if mode == UNIDIR else 2), (what, r)
    finally:
        P.close()
