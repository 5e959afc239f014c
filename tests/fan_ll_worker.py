"""Child processes of tests/test_gpu_fan_ll.py (MPX_TEST is the parent's choice):

    fan_ll_worker.py lag <nranks> <iters>    under MPX_TEST=lag_wg=1:0:<us>
    fan_ll_worker.py no_posted               under MPX_TEST=no_posted
    fan_ll_worker.py ipc <dir> <p>           one of two processes, a rank each

lag: a checked 4096-byte LL fan call on a full mesh whose rank 1 stalls link
workgroup 0 (its link to rank 0) between its push and its wait of iteration
iters / 2; prints the links' device_s.  no_posted: fan_ll.race with a bulk
second call; prints whether the sleeper's rx between the calls differed from
what call 1 left.  ipc: process p owns rank p of a 2-rank context on GPU 0,
imports the other and runs a checked 4095-byte LL exchange with it.
Each prints one JSON line.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mpi-perf_amd"))
sys.path.insert(0, HERE)
import mpx  # noqa: E402
import oracle_py as O  # noqa: E402
import payload  # noqa: E402
from fan import flat_image, full_mesh, round16  # noqa: E402
from fan_ll import RACE_N, SEED_B, mesh, race  # noqa: E402


def lag(nranks, iters):
    sets = full_mesh(nranks)
    F = mesh(nranks, 4096)
    try:
        out = F.checked_call(sets, iters, True, ("lag", nranks, iters))
        res = {f"{r}-{l['peer']}": l["device_s"] for r in sets for l in out[r][1]}
    finally:
        F.close()
    print(json.dumps(dict(ok=True, device_s=res)))


def no_posted():
    between, want = race(2, False, second_ll=False)
    early = flat_image(len(want), 0, SEED_B)[round16(RACE_N):round16(RACE_N) + RACE_N]
    print(json.dumps(dict(mismatch=between != want, early_block=between[:RACE_N] == early)))


def wait_for(path):
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > 60:
            raise SystemExit(f"{path} never appeared")
        time.sleep(0.01)


def ipc(d, p):
    n, iters, stride = 4095, 5, 4096
    cap = 2 * stride + payload.GUARD
    c = mpx.Context(2, "kernel")

    def image(r):
        h = bytearray(O.fill(cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 63, 1)))
        for dst in range(2):
            h[dst * stride:dst * stride + n] = O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, dst, 7))
        return bytes(h)

    tx, rx = c.alloc(0, cap), c.alloc(0, cap)
    payload.write(c, tx, image(p))
    c.fill(rx, cap, mpx.FILL_BYTE, payload.GUARD_BYTE)
    c.attach(p, 0, tx, rx, cap)
    with open(os.path.join(d, f"desc_{p}.tmp"), "wb") as f:
        f.write(c.export(p))
    os.rename(os.path.join(d, f"desc_{p}.tmp"), os.path.join(d, f"desc_{p}.bin"))
    q = 1 - p
    wait_for(os.path.join(d, f"desc_{q}.bin"))
    c.import_rank(q, open(os.path.join(d, f"desc_{q}.bin"), "rb").read())
    block = image(q)[p * stride:p * stride + n]
    s = O.checksum(block)
    before = c.link_counters(p, q)
    t, links = c.fan(p, [q], iters, tx, rx, n, stride, check_payload=True, expect=[s], timeout_ms=5000, ll=True)
    want = bytearray([payload.GUARD_BYTE]) * cap
    want[q * stride:q * stride + n] = block
    print(json.dumps(dict(rank=p, protocol=t.protocol, nwg=t.nwg, launches=t.launches, recv_done=t.recv_done,
                          check_iters=t.check_iters, check_failures=t.check_failures, bytes=t.bytes,
                          digest_ok=t.recv_digest == (iters * s) & 0xFFFFFFFFFFFFFFFF, links=links,
                          before=before, after=c.link_counters(p, q),
                          rx_ok=c.read(rx, cap) == bytes(want), tx_ok=c.read(tx, cap) == image(p))))
    # the other process may still poll this one's pushes: leave together
    open(os.path.join(d, f"done_{p}"), "w").close()
    wait_for(os.path.join(d, f"done_{q}"))
    c.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "lag":
        lag(int(sys.argv[2]), int(sys.argv[3]))
    elif mode == "no_posted":
        no_posted()
    else:
        ipc(sys.argv[2], int(sys.argv[3]))
