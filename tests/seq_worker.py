"""GPU worker for tests/test_gpu_seq.py: the cases that need a process of their
own, because libmpx reads what they depend on once per process.

  ring3     started with MPX_CHECK_RING_BYTES of two slots: the sequenced
            non-blocking loop in check mode with three receive slots per link,
            4097 B x 33
  pullenv   started with MPX_XFER_PULL=1: mpx_xfer_seq is refused
            (MPX_ERR_UNSUPPORTED) before anything moves, and ordinary calls of
            the same context go on working, pulled

Prints "ok" or raises.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "mpi-perf_amd"), HERE]
import mpx  # noqa: E402


def ring3():
    import hostpairs as W
    import payload
    import seq as S
    from wrap_worker import RING_BYTES_AT

    assert int(os.environ["MPX_CHECK_RING_BYTES"]) == W.CREDIT_RING
    X = W.HostPairs(W.CREDIT_CAP)
    try:
        out = S.verified(X, W.NONBLOCKING, W.CREDIT_N, 33, "three slots")
        assert [out[r].protocol for r in (0, 1)] == [1, 1]
        ring = int.from_bytes(X.c.export(0)[RING_BYTES_AT:RING_BYTES_AT + 8], "little")
        assert ring == payload.ring_bytes_for(W.CREDIT_CAP, W.CREDIT_RING), ring
        assert payload.ring_slots(ring, W.CREDIT_N) == 3
    finally:
        X.close()


def pullenv():
    import hostpairs as W
    import seq as S

    assert os.environ["MPX_XFER_PULL"] == "1"
    X = W.HostPairs(4161 + W.GUARD)
    try:
        before = [X.counters(r) for r in X.ranks]
        out, errs = S.run(X, W.PINGPONG, 4161, 3, check=False)
        assert not out and sorted(errs) == [0, 1], (out, errs)
        for e in errs.values():
            assert e.status == mpx.ERR_UNSUPPORTED and "MPX_XFER_PULL" in str(e), str(e)
        assert [X.counters(r) for r in X.ranks] == before
        out = W.run_checked(X, W.PINGPONG, 4161, 3, "pulled")
        assert out[0].protocol == 7
    finally:
        X.close()


if __name__ == "__main__":
    {"ring3": ring3, "pullenv": pullenv}[sys.argv[1]]()
    print("ok")
