"""GPU worker for tests/test_gpu_ranks.py: the cases that need a process of
their own, because libmpx reads MPX_CHECK_RING_BYTES once per process.  Both
start with it at hostpairs.CREDIT_RING (two slots of 4097 + GUARD bytes).

  credits   ranks 5, 37 and 63 of a 64-rank context, all attached with
            4097 + GUARD bytes: non-blocking check mode with three receive
            slots per link, on links at different counts, pushed and pulled,
            kernel and SDMA engines
  unequal   rank 5 attached with 4097 + GUARD bytes and rank 63 with 1 MiB:
            their rings give three slots and one; both ends of the link must
            use one (link_slots: the minimum), in either group order

Prints "ok" or raises.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "mpi-perf_amd"), HERE]
import hostpairs as W  # noqa: E402
import payload  # noqa: E402
from links import NONBLOCKING, PROTO_BULK, PROTO_PULL, PROTO_SDMA, PROTO_SDMA_PULL, Links, link  # noqa: E402

RING_BYTES_AT = 264       # offsetof(RankDesc, ring_bytes), as tests/wrap_worker.py reads it


def ring_of(X, r):
    """the ring this process really allocated for rank r, from its descriptor"""
    return int.from_bytes(X.c.export(r)[RING_BYTES_AT:RING_BYTES_AT + 8], "little")


def credits():
    for engine, push, pull in (("kernel", PROTO_BULK, PROTO_PULL), ("sdma", PROTO_SDMA, PROTO_SDMA_PULL)):
        X = Links(engine, [5, 37, 63], W.CREDIT_CAP)
        try:
            # ranks 37 and 5 are equal modulo 32: rank 63 meets them in this order with descending counts, so
            # what the first leaves in a shared row of credits would let the second run ahead of its slots
            X.advance(37, 63, seq_by=W.P32 + 3000, calls_by=9)
            X.advance(5, 63, seq_by=W.P32 - 7, calls_by=5)      # this link crosses push 2^32 inside the call
            X.advance(5, 37, seq_by=1000)
            for a, b in ((37, 63), (63, 5), (5, 37), (63, 37)):
                X.round([link(a, b, NONBLOCKING, W.CREDIT_N, 20, proto=push)], ("credits", engine, a, b))
                X.round([link(b, a, NONBLOCKING, W.CREDIT_N, 20, proto=pull, pull=True)],
                        ("credits pulled", engine, a, b))
            for r in X.ranks:
                ring = ring_of(X, r)
                assert ring == payload.ring_bytes_for(W.CREDIT_CAP, W.CREDIT_RING), (engine, r, ring)
                assert payload.ring_slots(ring, W.CREDIT_N) == 3
        finally:
            X.close()


def unequal():
    for engine, push in (("kernel", PROTO_BULK), ("sdma", PROTO_SDMA)):
        X = Links(engine, [5, 63], 1 << 20, caps={5: W.CREDIT_CAP})
        try:
            X.advance(5, 63, seq_by=77)
            for a, b in ((5, 63), (63, 5)):
                for n in (W.CREDIT_N, W.CREDIT_CAP, 1, 1400):
                    X.round([link(a, b, NONBLOCKING, n, 20, proto=push)], ("unequal rings", engine, a, b, n))
            rings = {r: ring_of(X, r) for r in X.ranks}
            assert rings == {5: payload.ring_bytes_for(W.CREDIT_CAP, W.CREDIT_RING),
                             63: payload.ring_bytes_for(1 << 20, W.CREDIT_RING)}, (engine, rings)
            assert [payload.ring_slots(rings[r], W.CREDIT_N) for r in (5, 63)] == [3, 1]
            assert [payload.ring_slots(rings[r], 1400) for r in (5, 63)] == [6, 1]
        finally:
            X.close()


if __name__ == "__main__":
    assert int(os.environ["MPX_CHECK_RING_BYTES"]) == W.CREDIT_RING
    {"credits": credits, "unequal": unequal}[sys.argv[1]]()
    print("ok")
