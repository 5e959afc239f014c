"""One rank of the 2-process IPC test (tests/test_gpu_ipc.py).

Each process owns one mpx context with one local rank on GPU 0, exports its
descriptor to a file, imports the other rank's, then runs every loop mode
with every payload checksummed.  Results go to <dir>/result_<rank>.json.

Two further arguments, <seq_by> <bytes> (tests/test_gpu_wrap.py): right after
attach and import each process advances its own side of the link by seq_by
pushes (mpx_test_advance_link), then runs one ping-pong and one unidir call
of 9 iterations of that size, and records the link's counters around each.

IPC_WORKER_RANKS="a,b" and IPC_WORKER_NRANKS (tests/test_gpu_ranks.py): the
two processes are ranks a (group 1) and b of a context of that many ranks;
<rank> stays 0 or 1 and names the files.  The engine "kernel-both" runs the
whole list pushed and then pulled.  Every result carries the link's counters
after its call, and whether every other row of the rank's counters is still
zero.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-perf_amd"))
import mpx  # noqa: E402


# 8191 / 8192 / 8193: both sides of the cross-GPU LL threshold (ll_max_bytes)
SIZES = (1, 8, 4097, 8191, 8192, 8193, 65541, 1 << 20)


def advanced(c, d, idx, rank, peer, group, tx, rx, peer_sums, seq_by, n):
    c.test_advance_link(rank, peer, seq_by, 0, 0)
    try:
        c.link_counters(peer, rank)
        imported = mpx.OK
    except mpx.MpxError as e:
        imported = e.status
    # the peer's tx, from the host's restatement of its fill
    import oracle_py as O
    theirs = O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, peer, rank, 0))
    assert O.checksum(theirs[:1]) == peer_sums["1"]
    results = []
    for mode in (mpx.MODE_PINGPONG, mpx.MODE_UNIDIR):
        before = c.link_counters(rank, peer)
        t = c.xfer(mode, group, rank, peer, 9, tx, rx, n, check_payload=True, expect=O.checksum(theirs),
                   expect_ack=O.checksum(theirs[:1]), timeout_ms=5000)
        m = 1 if (mode == mpx.MODE_UNIDIR and group == 1) else n
        results.append(dict(mode=mode, n=n, iters=9, check_iters=t.check_iters, check_failures=t.check_failures,
                            recv_done=t.recv_done, final_rx_ok=c.read(rx, m) == theirs[:m],
                            protocol=t.protocol, before=before, after=c.link_counters(rank, peer),
                            imported_rank_status=imported))
    with open(os.path.join(d, f"result_{idx}.json"), "w") as f:
        json.dump(results, f)


def main():
    d, idx = sys.argv[1], int(sys.argv[2])
    engine = sys.argv[3] if len(sys.argv) > 3 else "kernel"
    pull = engine.endswith("-pull")   # kernel-pull / sdma-pull: that engine in pull mode (MPX_XFER_PULL)
    both = engine.endswith("-both")
    engine = engine[:-len("-pull")] if pull or both else engine
    ids = [int(x) for x in os.environ.get("IPC_WORKER_RANKS", "0,1").split(",")]
    nranks = int(os.environ.get("IPC_WORKER_NRANKS", "2"))
    rank, peer = ids[idx], ids[1 - idx]
    # "cross": rank r on GPU r (the pair moves its bytes over xGMI); else GPU 0
    dev = idx if len(sys.argv) > 4 and sys.argv[4] == "cross" and not os.environ.get("MPX_MULTI_REHEARSE") else 0
    group = 1 if idx == 0 else 0
    cap = 1 << 20
    c = mpx.Context(nranks, engine)
    tx, rx = c.alloc(dev, cap), c.alloc(dev, cap)
    c.fill(tx, cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, rank, peer, 0))
    c.attach(rank, dev, tx, rx, cap)
    with open(os.path.join(d, f"desc_{idx}.tmp"), "wb") as f:
        f.write(c.export(rank))
    os.rename(os.path.join(d, f"desc_{idx}.tmp"), os.path.join(d, f"desc_{idx}.bin"))
    # my tx checksums, for the peer's expectations
    sums = {str(n): c.checksum(tx, n) for n in SIZES}
    with open(os.path.join(d, f"sums_{idx}.tmp"), "w") as f:
        json.dump(sums, f)
    os.rename(os.path.join(d, f"sums_{idx}.tmp"), os.path.join(d, f"sums_{idx}.json"))
    t0 = time.time()
    theirs = [os.path.join(d, f"desc_{1 - idx}.bin"), os.path.join(d, f"sums_{1 - idx}.json")]
    while not all(os.path.exists(f) for f in theirs):
        if time.time() - t0 > 60:
            raise SystemExit("peer never published its descriptor")
        time.sleep(0.01)
    c.import_rank(peer, open(os.path.join(d, f"desc_{1 - idx}.bin"), "rb").read())
    peer_sums = json.load(open(os.path.join(d, f"sums_{1 - idx}.json")))
    if len(sys.argv) > 6:
        advanced(c, d, idx, rank, peer, group, tx, rx, peer_sums, int(sys.argv[5]), int(sys.argv[6]))
        c.close()
        return
    results = []
    zero = dict(tx_seq=0, rx_seq=0, calls=0)
    for pull in ((False, True) if both else (pull,)):
        for mode in (mpx.MODE_PINGPONG, mpx.MODE_UNIDIR, mpx.MODE_NONBLOCKING):
            for n in SIZES:
                iters = 300 if mode == mpx.MODE_NONBLOCKING else 9
                t = c.xfer(mode, group, rank, peer, iters, tx, rx, n, check_payload=True,
                           expect=peer_sums[str(n)], expect_ack=peer_sums["1"], timeout_ms=5000, pull=pull)
                m = 1 if (mode == mpx.MODE_UNIDIR and group == 1) else n
                rows = {p: c.link_counters(rank, p) for p in range(nranks)}
                results.append(dict(mode=mode, n=n, iters=iters, check_iters=t.check_iters,
                                    check_failures=t.check_failures, recv_done=t.recv_done,
                                    final_rx_ok=c.checksum(rx, m) == peer_sums[str(m)], protocol=t.protocol,
                                    us_per_iter=t.wall_s / iters * 1e6, pull=pull, counters=rows[peer],
                                    other_rows_zero=all(dict(v, token=0) == dict(zero, token=0)
                                                        for p, v in rows.items() if p != peer)))
    with open(os.path.join(d, f"result_{idx}.json"), "w") as f:
        json.dump(results, f)
    c.close()


if __name__ == "__main__":
    main()
