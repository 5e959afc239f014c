"""Seeded, FREE-RUNNING soak of the fan exchange (mpx_xfer_fan) mixed with pair
calls on the same links: loopback ranks on GPU 0, one host thread per rank.

    python tools/fan_soak.py <steps> <seed> [nranks]      (MPX_TEST=no_posted: the negative control)

Every rank runs the whole plan on a thread of its own and never joins the
others between steps.  Before each of its calls a rank fills its rx with 0xEE
and writes its tx anew from the step's key; after it, it compares its WHOLE
rx (the peers' blocks of this step, 0xEE everywhere else) and its whole tx
with host bytes, and checks every field the call reports and its own side of
its link counters.  So a peer may already be inside step k + 1 while this rank
still reads step k's rx or prefills for k + 1: the situation the posted
handshake and check mode's credits exist for.  With the handshake off
(MPX_TEST=no_posted) the soak must report failures; that is what shows it can
see them.

A step is a fan step (a random symmetric peer graph, a random peer order per
rank, block length, stride, iterations, check, streaming stores, width) or a
checked pair call on one random edge (every loop; LL and bulk sizes); ranks
without an edge skip the step.  plan() is pure Python: tests/test_fan_soak_plan.py
holds it, for the seeds the GPU suite runs, to the limits a call accepts and
to covering everything listed here.

Buffers are written by the device (mpx_fill, the context's utility stream),
never by a host copy on the null stream, which could wait for the peers'
kernels.  Prints one JSON line; exit status 1 on any failure.
"""
import json
import os
import random
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "mpi-perf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK_LENS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4097, 16385, 65555]
MAX_BLOCK = 262144
FAN_ITERS = [0, 1, 2, 3, 15, 16, 17, 33, 64]
NWGS = [0, 1, 2, 7, 32]
PAIR_LENS = [0, 8, 2045, 4097, 65555]            # 0, 8, 2045: the LL path
PAIR_MODES = [0, 1, 2]                           # MPX_MODE_PINGPONG, _NONBLOCKING, _UNIDIR
GUARD = 64
M64 = 0xFFFFFFFFFFFFFFFF
# what tests/test_gpu_fan_soak.py runs on every pass of the GPU suite
SUITE_STEPS = 150
SUITE_SEEDS = (7, 12)


def round16(n):
    return (n + 15) & ~15


def room(nranks):
    """bytes of tx / rx every rank's block may take (a multiple of 16)"""
    return round16(MAX_BLOCK) + 4096


def capacity(nranks):
    return nranks * room(nranks) + GUARD


def plan(steps, seed, nranks=4):
    rng = random.Random(seed)
    out = []
    for k in range(steps):
        key = (seed * 4096 + k + 1) & 0xFFFFFF
        if rng.random() < 0.2:
            a, b = sorted(rng.sample(range(nranks), 2))
            out.append(dict(kind="pair", key=key, a=a, b=b, mode=rng.choice(PAIR_MODES), n=rng.choice(PAIR_LENS),
                            iters=rng.randint(1, 20)))
            continue
        edges = [(a, b) for a in range(nranks) for b in range(a + 1, nranks) if rng.random() < 0.6]
        if not edges:
            edges = [tuple(sorted(rng.sample(range(nranks), 2)))]
        peers = {}
        for r in range(nranks):
            mine = [b if a == r else a for a, b in edges if r in (a, b)]
            if mine:
                rng.shuffle(mine)
                peers[r] = mine
        n = rng.choice(BLOCK_LENS) if rng.random() < 0.7 else rng.randint(0, MAX_BLOCK)
        stride = round16(n)
        spare = (room(nranks) - stride) // 16
        if spare > 0 and rng.random() < 0.5:
            stride += 16 * rng.randint(1, spare)
        out.append(dict(kind="fan", key=key, peers=peers, n=n, stride=stride, iters=rng.choice(FAN_ITERS),
                        check=rng.random() < 0.6, stream=rng.random() < 0.3, nwg=rng.choice(NWGS)))
    return out


# ---- one rank's side --------------------------------------------------------
class Failures(list):
    """what went wrong, and how many calls were made and verified at all"""
    def __init__(self):
        super().__init__()
        self.marks = []
        self.done = []          # one entry per call made (list.append is atomic between the ranks' threads)

    def note(self, rank, k, step, what):
        self.append(dict(rank=rank, step=k, what=str(what)[:400],
                         plan={a: b for a, b in step.items() if a != "peers"} | {"peers": step.get("peers", {}).get(rank)}))


def _expect(cond, what):
    if not cond:
        raise AssertionError(what)


def expected_calls(steps, nranks=4):
    """calls the ranks make in all: two per pair step, one per rank with an edge per fan step"""
    return sum(2 if s["kind"] == "pair" else len(s["peers"]) for s in steps)


def run_rank(F, r, steps, fails):
    """rank r's side of the plan; anything it raises is a failure too"""
    try:
        _run_rank(F, r, steps, fails)
    except Exception as e:  # noqa: BLE001
        fails.note(r, -1, {}, f"rank {r}'s thread ended: {type(e).__name__}: {e}")


def _run_rank(F, r, steps, fails):
    """rank r's side of the plan on F (tests/fan.py Fan); stops at a timeout:
    the rank is broken and its links' state unknown afterwards"""
    import mpx
    import oracle_py as O
    import payload
    from fan import fan_width, flat_image
    tx, rx = F.bufs[r]
    others = [p for p in range(F.n) if p != r]
    guard = bytes([payload.GUARD_BYTE])

    def prepare(key):
        F.c.fill(rx, F.cap, mpx.FILL_BYTE, payload.GUARD_BYTE)
        F.fill_tx(r, key)

    def counters():
        return {p: F.c.link_counters(r, p) for p in others}

    def check_counters(before, on, iters):
        after = counters()
        for p in others:
            b, a = before[p], after[p]
            d = iters if p in on else 0
            _expect(a["tx_seq"] == b["tx_seq"] + d and a["rx_seq"] == b["rx_seq"] + d, ("push numbers", p, b, a))
            _expect(a["calls"] == b["calls"] + (1 if p in on and iters > 0 else 0), ("call number", p, b, a))
            _expect(a["token"] == b["token"] + 1, ("token", p, b, a))

    def check_buffers(want_rx, own):
        payload.compare(F.c.read(rx, F.cap), bytes(want_rx), 0, f"rx of rank {r}")
        payload.compare(F.c.read(tx, F.cap), own, 0, f"tx of rank {r}")

    for k, s in enumerate(steps):
        if r == 0 and k % max(1, len(steps) // 4) == 0:
            fails.marks.append(round(time.time(), 2))      # rank 0's clock at every quarter of the plan
        if s["kind"] == "pair":
            if r not in (s["a"], s["b"]):
                continue
            peer = s["b"] if r == s["a"] else s["a"]
            group = 1 if r == s["a"] else 0
            n, iters, mode = s["n"], s["iters"], s["mode"]
            m = 1 if (mode == mpx.MODE_UNIDIR and group == 1) else n
            theirs = flat_image(F.cap, peer, s["key"])
            prepare(s["key"])
            before = counters()
            try:
                t = F.c.xfer(mode, group, r, peer, iters, tx, rx, n, check_payload=True, expect=O.checksum(theirs[:n]),
                             expect_ack=O.checksum(theirs[:1]), timeout_ms=5000)
            except mpx.MpxError as e:
                fails.note(r, k, s, e)
                if e.status == mpx.ERR_TIMEOUT:
                    return
                fails.done.append(r)
                continue
            try:
                _expect(t.check_failures == 0 and t.check_iters == iters, ("pair check", t.as_dict()))
                check_buffers(bytearray(theirs[:m]) + bytearray(guard) * (F.cap - m), flat_image(F.cap, r, s["key"]))
                check_counters(before, [peer], iters)
            except AssertionError as e:
                fails.note(r, k, s, e)
            fails.done.append(r)
            continue
        peers = s["peers"].get(r)
        if not peers:
            continue
        n, stride, iters, check = s["n"], s["stride"], s["iters"], s["check"]
        blocks = [flat_image(F.cap, p, s["key"])[r * stride:r * stride + n] for p in peers]
        sums = [O.checksum(b) for b in blocks]
        prepare(s["key"])
        before = counters()
        try:
            t, links = F.c.fan(r, peers, iters, tx, rx, n, stride, check_payload=check, expect=sums, timeout_ms=5000,
                               nwg=s["nwg"], stream=s["stream"])
        except mpx.MpxError as e:
            fails.note(r, k, s, e)
            if e.status == mpx.ERR_TIMEOUT:
                return
            fails.done.append(r)
            continue
        try:
            want = bytearray(guard) * F.cap
            if iters > 0:
                for p, b in zip(peers, blocks):
                    want[p * stride:p * stride + n] = b
            check_buffers(want, flat_image(F.cap, r, s["key"]))
            width = fan_width(F.n, n, nwg=s["nwg"])
            np_ = len(peers)
            _expect(t.protocol == 9 and t.launches == 1 and t.nwg == width, ("protocol, launches, width", t.as_dict()))
            _expect(t.bytes == 2 * n * iters * np_ and t.recv_done == np_ * iters, ("bytes, receives", t.as_dict()))
            _expect(t.recv_digest == (sum(iters * x for x in sums) & M64 if check else 0), ("digest", t.as_dict()))
            _expect(t.check_failures == 0 and t.check_iters == (np_ * iters if check else 0), ("check", t.as_dict()))
            _expect(0 <= t.device_s < 5.0 and 0 <= t.wall_s < 5.0 + 1.0, ("times", t.as_dict()))
            _expect([l["peer"] for l in links] == list(peers), ("link order", links))
            for j, l in enumerate(links):
                _expect(l["nwg"] == width and l["recv_done"] == iters and l["check_failures"] == 0, ("link", l))
                _expect(l["recv_digest"] == ((iters * sums[j]) & M64 if check else 0), ("link digest", l))
                _expect(0 <= l["device_s"] < 5.0, ("link time", l))
            check_counters(before, peers, iters)
        except AssertionError as e:
            fails.note(r, k, s, e)
        fails.done.append(r)


def run(steps, seed, nranks=4):
    from fan import Fan
    todo = plan(steps, seed, nranks)
    t0 = time.time()
    F = Fan(nranks, capacity(nranks))
    fails = Failures()
    try:
        th = [threading.Thread(target=run_rank, args=(F, r, todo, fails)) for r in range(nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        F.close()
    kinds = {}
    for f in fails:
        w = f["what"]
        kind = ("timeout" if "timed out" in w else "check" if "failed the checksum" in w else
                "bytes" if "bytes differ" in w else "other")
        kinds[kind] = kinds.get(kind, 0) + 1
    return dict(tool="fan_soak", steps=steps, seed=seed, nranks=nranks, test_knobs=os.environ.get("MPX_TEST", ""),
                calls=len(fails.done), expected_calls=expected_calls(todo, nranks), failures=len(fails), kinds=kinds,
                first=list(fails[:4]), quarters_s=[round(b - a, 2) for a, b in zip(fails.marks, fails.marks[1:] + [time.time()])],
                seconds=round(time.time() - t0, 1))


if __name__ == "__main__":
    res = run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    print(json.dumps(res), flush=True)
    sys.exit(1 if res["failures"] or res["calls"] != res["expected_calls"] else 0)
