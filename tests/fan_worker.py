"""One process of the 2-process fan test (tests/test_gpu_fan.py).

Process p owns ranks 2p and 2p + 1 of a 4-rank context on GPU 0, exports both,
imports the other process's two, then every local rank (a thread each) runs a
checked full-mesh fan exchange: one link to the rank next door, two over
imported ranks.  tx is written from host bytes, seeded per (src, dst), so the
other process's blocks are known here without asking it; rx is 0xEE before
the call and compared whole after it.  Results go to <dir>/result_<p>.json.

An optional third argument jump=<next_push> (tests/test_gpu_fan_wrap.py): right
after attach and import, this process advances its own side of every link of
its ranks, the links to imported ranks included, so that the link's next push
is that number (mpx_test_advance_link: each process its own side); the link
counters before and after the call go into the result.
"""
import json
import os
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mpi-perf_amd"))
sys.path.insert(0, HERE)
import mpx  # noqa: E402
import oracle_py as O  # noqa: E402
import payload  # noqa: E402

WORLD, N, ITERS = 4, 65555, 3
STRIDE = (N + 15) & ~15
CAP = WORLD * STRIDE + payload.GUARD
M64 = 0xFFFFFFFFFFFFFFFF


def block(src, dst):
    return O.fill(N, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, src, dst, 7))


def wait_for(path):
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > 60:
            raise SystemExit(f"{path} never appeared")
        time.sleep(0.01)


def main():
    d, p = sys.argv[1], int(sys.argv[2])
    jump = int(sys.argv[3].split("=", 1)[1]) if len(sys.argv) > 3 and sys.argv[3].startswith("jump=") else 0
    mine = [2 * p, 2 * p + 1]
    theirs = [r for r in range(WORLD) if r not in mine]
    c = mpx.Context(WORLD, "kernel")
    bufs, host = {}, {}
    for r in mine:
        tx, rx = c.alloc(0, CAP), c.alloc(0, CAP)
        h = bytearray(O.fill(CAP, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 63, 1)))
        for dst in range(WORLD):
            h[dst * STRIDE:dst * STRIDE + N] = block(r, dst)
        host[r] = bytes(h)
        payload.write(c, tx, host[r])
        c.fill(rx, CAP, mpx.FILL_BYTE, payload.GUARD_BYTE)
        c.attach(r, 0, tx, rx, CAP)
        bufs[r] = (tx, rx)
    for r in mine:
        with open(os.path.join(d, f"desc_{r}.tmp"), "wb") as f:
            f.write(c.export(r))
        os.rename(os.path.join(d, f"desc_{r}.tmp"), os.path.join(d, f"desc_{r}.bin"))
    for r in theirs:
        wait_for(os.path.join(d, f"desc_{r}.bin"))
        c.import_rank(r, open(os.path.join(d, f"desc_{r}.bin"), "rb").read())
    if jump:
        for r in mine:
            for q in range(WORLD):
                if q != r:
                    c.test_advance_link(r, q, jump - 1, 0, 0)
    results, errs = [], []

    def side(r):
        peers = [q for q in range(WORLD) if q != r]
        if r % 2:
            peers.reverse()
        sums = [O.checksum(block(q, r)) for q in peers]
        before = {q: c.link_counters(r, q) for q in peers}
        try:
            t, links = c.fan(r, peers, ITERS, bufs[r][0], bufs[r][1], N, STRIDE, check_payload=True, expect=sums,
                             timeout_ms=20000)
        except mpx.MpxError as e:
            errs.append((r, str(e)))
            return
        want = bytearray([payload.GUARD_BYTE]) * CAP
        for q in peers:
            want[q * STRIDE:q * STRIDE + N] = block(q, r)
        results.append(dict(rank=r, iters=ITERS, check_iters=t.check_iters, check_failures=t.check_failures,
                            recv_done=t.recv_done, protocol=t.protocol, links=links,
                            before=[before[q] for q in peers], after=[c.link_counters(r, q) for q in peers],
                            digest_ok=t.recv_digest == sum(ITERS * s for s in sums) & M64,
                            rx_ok=c.read(bufs[r][1], CAP) == bytes(want), tx_ok=c.read(bufs[r][0], CAP) == host[r]))

    th = [threading.Thread(target=side, args=(r,)) for r in mine]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise SystemExit(f"fan calls failed: {errs}")
    with open(os.path.join(d, f"result_{p}.json"), "w") as f:
        json.dump(results, f)
    # the other process may still push into this one's rx and mailboxes: leave together
    open(os.path.join(d, f"done_{p}"), "w").close()
    wait_for(os.path.join(d, f"done_{1 - p}"))
    c.close()


if __name__ == "__main__":
    main()
