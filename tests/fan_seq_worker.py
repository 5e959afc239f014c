"""Child processes of tests/test_gpu_fan_seq.py:

    fan_seq_worker.py lost <bulk|ll>     started with MPX_TEST=skip_push=<k>
    fan_seq_worker.py ipc <bulk|ll> <dir> <p>   one of two processes, a rank each

lost: a 3-iteration sequenced fan call on a full mesh of 3 with push k of
every link "lost" (no payload stores, the flag or the tags still go).
skip_push=3, unchecked (bulk): the call completes and every rx block holds the
payload of iteration 1.  skip_push=2, checked: MPX_ERR_CHECK with exactly one
failure per link.
ipc: process p owns rank p of a 2-rank context on GPU 0, imports the other and
runs a checked sequenced exchange with it, whose bytes it compares whole.
Each prints one JSON line.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "mpi-perf_amd"), HERE]
import mpx  # noqa: E402
import oracle_py as O  # noqa: E402
import payload  # noqa: E402
import fan_seq as S  # noqa: E402
from fan import full_mesh  # noqa: E402


def lost(kind):
    ll = kind == "ll"
    k = int(os.environ["MPX_TEST"].split("=", 1)[1])
    n = 2045 if ll else 4161
    sets = full_mesh(3)
    F = S.mesh(3, n)
    try:
        if k == 3:      # the last push is lost, nobody checks: the bytes of iteration 1 stay
            out, errs = S.run(F, sets, 3, check=False, ll=ll)
            assert not errs, errs
            assert not ll and all(out[r][0].recv_done == 6 for r in sets), out
            S.verify_bytes(F, sets, 1, "skip_push=3")
            res = dict(ok=True)
        else:           # push k is lost and every payload is checked: one failure per link
            out, errs = S.run(F, sets, 3, check=True, ll=ll)
            assert not out and sorted(errs) == [0, 1, 2], (out, errs)
            for r, e in errs.items():
                assert e.status == mpx.ERR_CHECK, (r, str(e))
                assert e.timing.check_failures == 2 and e.timing.check_iters == 6, (r, e.timing.check_failures)
                assert [l["check_failures"] for l in e.links] == [1, 1], (r, e.links)
            res = dict(ok=True)
    finally:
        F.close()
    print(json.dumps(res))


def wait_for(path):
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > 60:
            raise SystemExit(f"{path} never appeared")
        time.sleep(0.01)


def ipc(kind, d, p):
    ll = kind == "ll"
    n, iters = (4095, 5) if ll else (65555, 3)
    stride = ((n + 15) & ~15) + 16
    cap = 2 * stride + payload.GUARD
    c = mpx.Context(2, "kernel")
    image = O.fill(cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, p, 63, 1))
    tx, rx = c.alloc(0, cap), c.alloc(0, cap)
    payload.write(c, tx, image)
    c.fill(rx, cap, mpx.FILL_BYTE, payload.GUARD_BYTE)
    c.attach(p, 0, tx, rx, cap)
    with open(os.path.join(d, f"desc_{p}.tmp"), "wb") as f:
        f.write(c.export(p))
    os.rename(os.path.join(d, f"desc_{p}.tmp"), os.path.join(d, f"desc_{p}.bin"))
    q = 1 - p
    wait_for(os.path.join(d, f"desc_{q}.bin"))
    c.import_rank(q, open(os.path.join(d, f"desc_{q}.bin"), "rb").read())
    before = c.link_counters(p, q)
    t, links = c.xfer_fan_seq(p, [q], iters, tx, rx, n, stride, S.SEED, check_payload=True,
                              expect=S.expectations(p, [q], n, iters), timeout_ms=5000, ll=ll)
    S.check_rx(c.read(rx, cap), cap, stride, n, p, [q], iters - 1, f"ipc {kind}, process {p}")
    digest = sum(S.csum(S.SEED, q, p, i, n) for i in range(iters)) & S.M64
    print(json.dumps(dict(rank=p, protocol=t.protocol, launches=t.launches, recv_done=t.recv_done,
                          check_iters=t.check_iters, check_failures=t.check_failures, bytes=t.bytes,
                          digest_ok=t.recv_digest == digest == links[0]["recv_digest"], links=links,
                          before=before, after=c.link_counters(p, q), tx_ok=c.read(tx, cap) == image)))
    # the other process may still poll or push: leave together
    open(os.path.join(d, f"done_{p}"), "w").close()
    wait_for(os.path.join(d, f"done_{q}"))
    c.close()


if __name__ == "__main__":
    if sys.argv[1] == "lost":
        lost(sys.argv[2])
    else:
        ipc(sys.argv[2], sys.argv[3], int(sys.argv[4]))
