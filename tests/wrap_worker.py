"""GPU worker for tests/test_gpu_wrap.py: the cases that need a process of
their own, because libmpx reads what they depend on once per process.

  nogate    started WITHOUT MPX_TEST in the environment: mpx_test_advance_link
            returns MPX_ERR_UNSUPPORTED and moves nothing, mpx_link_counters
            works, and setting MPX_TEST later does not open the gate
  credits   started with MPX_CHECK_RING_BYTES of two slots: non-blocking check
            mode with three receive slots per link, 20 iterations from near
            2^31 and near 2^32, pushed and pulled

Prints "ok" or raises.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "mpi-perf_amd"), HERE]
import mpx  # noqa: E402

RING_BYTES_AT = 264       # offsetof(RankDesc, ring_bytes): magic, 4 ints, pid, len, bus id, host, two IPC handles


def nogate():
    assert "MPX_TEST" not in os.environ
    with mpx.Context(2, "kernel") as c:
        for r in (0, 1):
            tx, rx = c.alloc(0, 4096), c.alloc(0, 4096)
            c.attach(r, 0, tx, rx, 4096)
        zero = dict(tx_seq=0, rx_seq=0, calls=0, token=0)
        for setenv in (False, True):
            if setenv:      # the gate was read when the process started
                os.environ["MPX_TEST"] = ""
            try:
                c.test_advance_link(0, 1, 1, 1, 1)
            except mpx.MpxError as e:
                assert e.status == mpx.ERR_UNSUPPORTED, e
            else:
                raise AssertionError("mpx_test_advance_link worked without the MPX_TEST gate")
            assert c.link_counters(0, 1) == zero and c.link_counters(1, 0) == zero


def credits():
    import hostpairs as W
    import payload
    from hostpairs import NONBLOCKING, HostPairs

    assert int(os.environ["MPX_CHECK_RING_BYTES"]) == W.CREDIT_RING
    for pull in (False, True):
        X = HostPairs(W.CREDIT_CAP)
        try:
            for P in (W.P31, W.P32):
                W.jump(X, P - 4)
                out = W.checked(X, NONBLOCKING, W.CREDIT_N, 20, ("credits", P, pull), pull=pull)
                assert [out[r].protocol for r in (0, 1)] == [7 if pull else 1] * 2      # pull, bulk
                assert X.counters(0)["tx_seq"] == P + 15
            # the ring this process really allocated, from the rank's descriptor
            # (RankDesc.ring_bytes, mpx_runtime.hip), not from the variable
            ring = int.from_bytes(X.c.export(0)[RING_BYTES_AT:RING_BYTES_AT + 8], "little")
            assert ring == payload.ring_bytes_for(W.CREDIT_CAP, W.CREDIT_RING), (pull, ring)
            assert payload.ring_slots(ring, W.CREDIT_N) == 3
        finally:
            X.close()


if __name__ == "__main__":
    {"nogate": nogate, "credits": credits}[sys.argv[1]]()
    print("ok")
