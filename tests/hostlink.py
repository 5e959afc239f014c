"""Host links of one process, for tests/test_gpu_hostlink.py.

TEST INFRASTRUCTURE.  `npairs` GPU ranks [0, np) on GPU 0, each paired with a
host endpoint of its own, np + k (include/mpx_hostlink.h).  Every buffer is
attached `slack` bytes longer than the message size the link is built for; tx
holds host bytes this module seeded (oracle_py.fill, one key per rank), so
every expectation is built on the host from those bytes.  Each side of a call
runs on a thread of its own, like tests/pairs.py; the threads are joined with
a time limit, and a side that is still running then fails the test instead of
blocking it.
"""
from __future__ import annotations

import ctypes as C
import threading
import time

import mpx
import oracle_py
import payload

SLACK = 4096
GUARD_BYTE = 0xEE
JOIN_S = 30.0


class HostLinks:
    def __init__(self, n: int, npairs: int = 1, slack: int = SLACK):
        self.np = npairs
        self.cap = n + slack
        self.c = mpx.Context(2 * npairs, "kernel")
        self.tx_bytes = {}     # rank -> the host bytes its tx holds
        self.gpu = {}          # GPU rank -> (tx, rx) device buffers
        self.host = {}         # host endpoint -> (tx, rx) ctypes arrays over its pinned memory
        for r in range(2 * npairs):
            data = oracle_py.fill(self.cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 0, 0))
            self.tx_bytes[r] = data
            if r < npairs:
                tx, rx = self.c.alloc(0, self.cap), self.c.alloc(0, self.cap)
                payload.write(self.c, tx, data)
                self.c.attach(r, 0, tx, rx, self.cap)
                self.gpu[r] = (tx, rx)
            else:
                self.c.host_attach(r, self.cap)
                tx, rx = self.c.host_buffers(r)
                C.memmove(tx, data, self.cap)
                self.host[r] = (tx, rx)
        self.reset_rx()

    def peer(self, r: int) -> int:
        return r + self.np if r < self.np else r - self.np

    def reset_rx(self) -> None:
        """every rx back to the guard byte (between calls only)"""
        for tx, rx in self.gpu.values():
            self.c.fill(rx, self.cap, mpx.FILL_BYTE, GUARD_BYTE)
        for tx, rx in self.host.values():
            C.memset(rx, GUARD_BYTE, self.cap)

    def rx(self, r: int) -> bytes:
        """all of rank r's rx, as host bytes"""
        if r < self.np:
            return self.c.read(self.gpu[r][1], self.cap)
        return bytes(self.host[r][1])

    def expect(self, r: int, n: int):
        """(checksum of the peer's tx[0:n), checksum of its tx[0:1)): host bytes, the oracle's checksum"""
        data = self.tx_bytes[self.peer(r)]
        return oracle_py.checksum(data[:n]), oracle_py.checksum(data[:1])

    def want_rx(self, r: int, mode: int, group: int, n: int, iters: int) -> bytes:
        """what rank r's rx holds after a call from the guard state: the
        received range (the unidir sender's: the one ack byte), then guards"""
        got = 0 if iters == 0 else (1 if (mode == mpx.MODE_UNIDIR and group == 1) else n)
        return self.tx_bytes[self.peer(r)][:got] + bytes([GUARD_BYTE]) * (self.cap - got)

    def run(self, mode: int, gpu_group: int, n: int, iters: int, check: bool = False, nwg: int = 0,
            timeout_ms: int = 5000, pairs=None, delay=None, before=None):
        """Every side of the pairs `pairs` (default: all) on a thread of its
        own.  delay: {rank: seconds} a side sleeps before it enters; before:
        {rank: callable} run on that side's thread right before it enters,
        its result kept in self.seen[rank].  Returns (timings, errors) by
        rank; raises if a side is still running after JOIN_S."""
        pairs = list(range(self.np)) if pairs is None else list(pairs)
        out, errs, self.seen = {}, {}, {}

        def side(r: int) -> None:
            gpu_side = r < self.np
            group = gpu_group if gpu_side else 1 - gpu_group
            exp, ack = self.expect(r, n)
            kw = dict(check_payload=check, expect=exp, expect_ack=ack, timeout_ms=timeout_ms, nwg=nwg)
            if delay and r in delay:
                time.sleep(delay[r])
            if before and r in before:
                self.seen[r] = before[r]()
            try:
                if gpu_side:
                    out[r] = self.c.xfer_hostlink(mode, group, r, self.peer(r), iters, *self.gpu[r], n, **kw)
                else:
                    out[r] = self.c.host_xfer(mode, group, r, self.peer(r), iters, n, **kw)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,), daemon=True) for k in pairs for r in (k, k + self.np)]
        for t in th:
            t.start()
        deadline = time.monotonic() + JOIN_S
        for t in th:
            t.join(max(0.0, deadline - time.monotonic()))
        if any(t.is_alive() for t in th):
            raise AssertionError(f"a side of the host link is still running after {JOIN_S} s (lost hand-off)")
        return out, errs

    def close(self) -> None:
        self.c.close()


# ---- an explicit map of links (tests/test_gpu_hostlink_{wrap,forms,ranks,soak}.py) --
P31, P32 = 1 << 31, 1 << 32
M64 = (1 << 64) - 1
PAIR_LL_MAX = 2048     # loopback pairs switch from LL to bulk above 2 KiB
COUNTER_KEYS = ("tx_seq", "rx_seq", "calls")


class LinkMap:
    """A context of `nranks` ranks with the GPU ranks `gpu` (all on GPU 0) and
    the host endpoints `host` attached, and the links `links`, (gpu_rank,
    host_rank) pairs; a rank may appear in several links.  Every buffer is
    attached n + slack bytes; tx_bytes[r] is what rank r's tx holds (one seed
    per rank, set_tx draws it anew), so every expectation is host bytes.
    Every GPU rank is an ordinary local rank too: pair() and fan() run pair
    and fan calls between them on the same tx / rx."""

    def __init__(self, n: int, nranks: int, gpu, host, links, slack: int = SLACK):
        self.nranks, self.cap = nranks, n + slack
        self.gpu_ranks, self.host_ranks = list(gpu), list(host)
        self.links = [tuple(l) for l in links]
        assert not set(self.gpu_ranks) & set(self.host_ranks)
        assert all(g in self.gpu_ranks and h in self.host_ranks for g, h in self.links), self.links
        self.c = mpx.Context(nranks, "kernel")
        self.tx_bytes, self.gpu, self.host, self.seen = {}, {}, {}, {}
        for r in self.gpu_ranks:
            tx, rx = self.c.alloc(0, self.cap), self.c.alloc(0, self.cap)
            self.c.attach(r, 0, tx, rx, self.cap)
            self.gpu[r] = (tx, rx)
        for r in self.host_ranks:
            self.c.host_attach(r, self.cap)
            self.host[r] = self.c.host_buffers(r)
        for r in self.gpu_ranks + self.host_ranks:
            self.set_tx(r, 0)
        self.reset_rx()

    def close(self) -> None:
        self.c.close()

    def attached(self):
        return self.gpu_ranks + self.host_ranks

    def set_tx(self, r: int, seed: int) -> None:
        """rank r's whole tx drawn anew from the host (between calls): the
        GPU's with payload.write, an endpoint's with memmove"""
        data = oracle_py.fill(self.cap, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 0, seed & 0xFFFFFF))
        assert data != self.tx_bytes.get(r)
        self.tx_bytes[r] = data
        if r in self.gpu:
            payload.write(self.c, self.gpu[r][0], data)
        else:
            C.memmove(self.host[r][0], data, self.cap)

    def reset_rx(self, ranks=None) -> None:
        for r in self.attached() if ranks is None else ranks:
            if r in self.gpu:
                self.c.fill(self.gpu[r][1], self.cap, mpx.FILL_BYTE, GUARD_BYTE)
            else:
                C.memset(self.host[r][1], GUARD_BYTE, self.cap)

    def rx(self, r: int) -> bytes:
        return self.c.read(self.gpu[r][1], self.cap) if r in self.gpu else bytes(self.host[r][1])

    def tx(self, r: int) -> bytes:
        return self.c.read(self.gpu[r][0], self.cap) if r in self.gpu else bytes(self.host[r][0])

    def blank(self) -> bytes:
        return bytes([GUARD_BYTE]) * self.cap

    def expect(self, r: int, peer: int, n: int):
        data = self.tx_bytes[peer]
        return oracle_py.checksum(data[:n]), oracle_py.checksum(data[:1])

    @staticmethod
    def got(mode: int, group: int, n: int, iters: int) -> int:
        """bytes a side of that group receives per message (0: none at all)"""
        return 0 if iters == 0 else (1 if (mode == mpx.MODE_UNIDIR and group == 1) else n)

    def want_rx(self, r: int, peer: int, mode: int, group: int, n: int, iters: int) -> bytes:
        k = self.got(mode, group, n, iters)
        return self.tx_bytes[peer][:k] + bytes([GUARD_BYTE]) * (self.cap - k)

    # ---- calls ------------------------------------------------------------------
    def run(self, links, mode: int, gpu_group: int, n: int, iters: int, check: bool = True, nwg: int = 0,
            timeout_ms: int = 5000, stage: bool = True, delay=None, before=None, also=()):
        """Both sides of every link of `links` on threads of their own, all
        with the same arguments.  Two links that share an end cannot run at
        once: an end has one rx.  delay / before: by rank, as HostLinks.run;
        also: further callables, each on a thread beside them (its result in
        self.also_out).  Returns ({(link, rank): Timing}, {(link, rank): MpxError})."""
        links = [tuple(l) for l in links]
        ends = [r for l in links for r in l]
        if len(set(ends)) != len(ends):
            raise ValueError(f"links {links} share an end: one rx cannot serve two calls at once")
        assert all(l in self.links for l in links), links
        out, errs, self.seen, self.also_out = {}, {}, {}, {}

        def side(link, r) -> None:
            g, h = link
            gpu_side = r == g
            group = gpu_group if gpu_side else 1 - gpu_group
            exp, ack = self.expect(r, h if gpu_side else g, n)
            kw = dict(check_payload=check, expect=exp, expect_ack=ack, timeout_ms=timeout_ms, nwg=nwg)
            if delay and r in delay:
                time.sleep(delay[r])
            if before and r in before:
                self.seen[r] = before[r]()
            try:
                if gpu_side:
                    out[link, r] = self.c.xfer_hostlink(mode, group, g, h, iters, *self.gpu[g], n, stage=stage, **kw)
                else:
                    out[link, r] = self.c.host_xfer(mode, group, h, g, iters, n, **kw)
            except mpx.MpxError as e:
                errs[link, r] = e

        def other(k, fn) -> None:
            try:
                self.also_out[k] = fn()
            except BaseException as e:  # noqa: BLE001 (the caller's to look at)
                self.also_out[k] = e

        th = [threading.Thread(target=side, args=(l, r), daemon=True) for l in links for r in l]
        th += [threading.Thread(target=other, args=(k, fn), daemon=True) for k, fn in enumerate(also)]
        for t in th:
            t.start()
        deadline = time.monotonic() + JOIN_S
        for t in th:
            t.join(max(0.0, deadline - time.monotonic()))
        if any(t.is_alive() for t in th):
            raise AssertionError(f"a side of the host link is still running after {JOIN_S} s (lost hand-off)")
        return out, errs

    def verify(self, out, links, mode, gpu_group, n, iters, check, what="", ll_max=None, rx_reset=True):
        """every byte of both ends' rx and tx, and everything the call reported"""
        ll_max = mpx.hostlink_ll_max() if ll_max is None else ll_max
        for link in links:
            g, h = link
            for r, peer, group in ((g, h, gpu_group), (h, g, 1 - gpu_group)):
                t = out[tuple(link), r]
                w = f"{what}: link {link} rank {r} ({'GPU' if r == g else 'host'}, group {group}) mode {mode} n {n} iters {iters}"
                if rx_reset:
                    payload.compare(self.rx(r), self.want_rx(r, peer, mode, group, n, iters), 0, w + " rx")
                payload.compare(self.tx(r), self.tx_bytes[r], 0, w + " tx")
                assert t.recv_done == iters, w
                assert t.bytes == n * iters * (1 if mode == mpx.MODE_UNIDIR else 2), w
                assert t.launches == (1 if r == g else 0), w
                assert t.protocol == (mpx.PROTO_HOSTLINK_LL if n <= ll_max else mpx.PROTO_HOSTLINK_BULK), w
                if check:
                    exp, ack = self.expect(r, peer, n)
                    want = ack if (mode == mpx.MODE_UNIDIR and group == 1) else exp
                    assert t.check_failures == 0 and t.check_iters == iters, (w, t.check_failures, t.check_iters)
                    assert t.recv_digest == (want * iters) & M64, w
                else:
                    assert t.check_iters == 0 and t.recv_digest == 0 and t.check_failures == 0, w

    def call(self, links, mode, gpu_group, n, iters, check=True, what="", ll_max=None, **kw):
        """reset every rx, run, no error on any side, verify; counted"""
        links = [tuple(l) for l in links]

        def go():
            self.reset_rx()
            out, errs = self.run(links, mode, gpu_group, n, iters, check=check, **kw)
            assert not errs, (what, {k: str(e) for k, e in errs.items()})
            self.verify(out, links, mode, gpu_group, n, iters, check, what, ll_max)
            self.untouched([r for l in links for r in l], what)
            return out
        return self.counted(links, iters, go, what)

    def untouched(self, used, what="") -> None:
        """rx of every attached rank outside `used` still holds the guard state"""
        for r in self.attached():
            if r not in used:
                payload.compare(self.rx(r), self.blank(), 0, f"{what}: rx of rank {r}, which took no part")

    # ---- pair and fan calls of the GPU ranks, on the same buffers -----------------
    def pair(self, a: int, b: int, mode: int, n: int, iters: int, check: bool = True, armed=False, what="", **kw):
        """a blocking pair call between GPU ranks a (group 1) and b, checked
        against host bytes; counted (armed: each side arms, then starts)"""
        def go():
            self.reset_rx()
            out, errs = {}, {}
            bar = threading.Barrier(2)

            def side(r, peer, group):
                exp, ack = self.expect(r, peer, n)
                args = (mode, group, r, peer, iters, *self.gpu[r], n)
                k = dict(check_payload=check, expect=exp, expect_ack=ack, timeout_ms=5000, **kw)
                try:
                    if armed:
                        self.c.arm(*args, **k)
                        bar.wait(JOIN_S)
                    out[r] = self.c.xfer(*args, **k)
                except mpx.MpxError as e:
                    errs[r] = e
                    bar.abort()
            th = [threading.Thread(target=side, args=x, daemon=True) for x in ((a, b, 1), (b, a, 0))]
            for t in th:
                t.start()
            for t in th:
                t.join(JOIN_S)
            assert not any(t.is_alive() for t in th), f"{what}: a side of the pair call is still running"
            assert not errs, (what, {k: str(e) for k, e in errs.items()})
            for r, peer, group in ((a, b, 1), (b, a, 0)):
                t = out[r]
                payload.compare(self.rx(r), self.want_rx(r, peer, mode, group, n, iters), 0, f"{what}: pair rx of rank {r}")
                payload.compare(self.tx(r), self.tx_bytes[r], 0, f"{what}: pair tx of rank {r}")
                assert t.recv_done == iters and t.launches == 1, (what, r, t.as_dict())
                if mode != mpx.MODE_UNIDIR or group == 1:      # (the side that sends the n bytes)
                    assert mpx.PROTOCOLS[t.protocol] == ("ll" if n <= PAIR_LL_MAX else "bulk"), (what, r, t.as_dict())
                if check:
                    exp, ack = self.expect(r, peer, n)
                    want = ack if (mode == mpx.MODE_UNIDIR and group == 1) else exp
                    assert t.check_failures == 0 and t.check_iters == iters, (what, r, t.as_dict())
                    assert t.recv_digest == (want * iters) & M64, (what, r)
            self.untouched((a, b), what)
            return out
        moves = {(a, b): (iters, 1 if iters else 0), (b, a): (iters, 1 if iters else 0)}
        return self.counted_moves(moves, {a: 1, b: 1}, go, what)

    def fan(self, ranks, block_len: int, stride: int, iters: int, what=""):
        """a checked fan exchange in the full mesh of the GPU ranks `ranks`:
        rank r's tx block p lands in rank p's rx block r; counted"""
        ranks = list(ranks)

        def go():
            self.reset_rx()
            out, errs = {}, {}

            def blk(src, dst):
                return self.tx_bytes[src][dst * stride:dst * stride + block_len]

            def side(r):
                peers = [p for p in ranks if p != r]
                try:
                    out[r] = self.c.fan(r, peers, iters, *self.gpu[r], block_len, stride, check_payload=True,
                                        expect=[oracle_py.checksum(blk(p, r)) for p in peers], timeout_ms=5000)
                except mpx.MpxError as e:
                    errs[r] = e
            th = [threading.Thread(target=side, args=(r,), daemon=True) for r in ranks]
            for t in th:
                t.start()
            for t in th:
                t.join(JOIN_S)
            assert not any(t.is_alive() for t in th), f"{what}: a side of the fan call is still running"
            assert not errs, (what, {k: str(e) for k, e in errs.items()})
            for r in ranks:
                want = bytearray(self.blank())
                for p in ranks:
                    if p != r and iters:
                        want[p * stride:p * stride + block_len] = blk(p, r)
                payload.compare(self.rx(r), bytes(want), 0, f"{what}: fan rx of rank {r}")
                payload.compare(self.tx(r), self.tx_bytes[r], 0, f"{what}: fan tx of rank {r}")
                t, links = out[r]
                assert t.check_failures == 0 and t.recv_done == iters * (len(ranks) - 1), (what, r, t.as_dict())
            self.untouched(ranks, what)
            return out
        moves = {(r, p): (iters, 1 if iters else 0) for r in ranks for p in ranks if p != r}
        return self.counted_moves(moves, {r: 1 for r in ranks}, go, what)

    # ---- the links' counters (mpx_link_counters, mpx_test_advance_link) -----------
    def counters(self, a: int, b: int) -> dict:
        """rank a's counters towards rank b: tx_seq, rx_seq, calls, token"""
        return self.c.link_counters(a, b)

    def all_counters(self) -> dict:
        """every attached rank towards every rank number of the context"""
        return {(a, b): self.counters(a, b) for a in self.attached() for b in range(self.nranks)}

    def jump(self, link, next_push: int) -> None:
        """both ends of the link: its next push is number `next_push`"""
        g, h = link
        c = [self.counters(g, h), self.counters(h, g)]
        last = c[0]["tx_seq"]
        assert all(x["tx_seq"] == last and x["rx_seq"] == last for x in c), c
        assert next_push - 1 > last
        for a, b in ((g, h), (h, g)):
            self.c.test_advance_link(a, b, next_push - 1 - last, 0, 0)
            x = self.counters(a, b)
            assert x["tx_seq"] == x["rx_seq"] == next_push - 1, x

    def advance(self, link, calls_by: int = 0, seq_by: int = 0) -> None:
        """both ends of the link forward alike"""
        g, h = link
        for a, b in ((g, h), (h, g)):
            self.c.test_advance_link(a, b, seq_by, calls_by, 0)

    def advance_token(self, g: int, by: int) -> None:
        peer = next(h for a, h in self.links if a == g)
        self.c.test_advance_link(g, peer, 0, 0, by)

    def counted_moves(self, moves: dict, tokens: dict, call, what=""):
        """call(), then EVERY counter of every attached rank towards every rank
        number: moves[(a, b)] = (pushes, calls) added to a's counters towards
        b, tokens[rank] added to a GPU rank's token; everything else — every
        other link of either end, every other rank — must read as before, and
        a host endpoint's token 0."""
        was = self.all_counters()
        out = call()
        now = self.all_counters()
        for (a, b), w in was.items():
            seq, calls = moves.get((a, b), (0, 0))
            want = dict(tx_seq=w["tx_seq"] + seq, rx_seq=w["rx_seq"] + seq, calls=w["calls"] + calls,
                        token=0 if a in self.host else w["token"] + tokens.get(a, 0))
            assert now[a, b] == want, (what, f"counters of rank {a} towards {b}", w, now[a, b], want)
        return out

    def counted(self, links, iters: int, call, what=""):
        """a host-link call on `links`: both ends' tx_seq and rx_seq moved by
        iters and calls by one (iters > 0), only the GPU end's token moved (by
        one), and no other link of either end moved"""
        moves, tokens = {}, {}
        for g, h in links:
            moves[g, h] = moves[h, g] = (iters, 1 if iters > 0 else 0)
            tokens[g] = tokens.get(g, 0) + 1
        return self.counted_moves(moves, tokens, call, what)


# ---- the seeded sequence soak (tests/test_gpu_hostlink_soak.py, test_hostlink_soak_plan.py) --
SOAK_SEEDS = (20251, 1003)   # (tests/test_hostlink_soak_plan.py: both plans reach every form)
SOAK_STEPS = 100
SOAK_GPU, SOAK_HOST, SOAK_LINKS = (0, 1), (2, 3), ((0, 2), (1, 3))
SOAK_WIDTHS = (0, 7, 70)


def soak_sizes(ll_max: int):
    return (0, 1, 8, ll_max, ll_max + 1, 2045, 4161, 71681)


def soak_plan(seed: int, steps: int = SOAK_STEPS, ll_max: int = 256):
    """the soak's steps, from the seed alone (random.Random: the same on every
    box).  kind: "a" = link (0, 2), "b" = link (1, 3), "both" = the two at
    once, "pair" = a blocking pair call between ranks 0 and 1.  reseed: the
    rank whose tx is drawn anew before the step."""
    import random
    rng = random.Random(seed)
    sizes = soak_sizes(ll_max)
    plan = []
    for k in range(steps):
        plan.append(dict(step=k, kind=rng.choice(("a", "b", "both", "pair")),
                         mode=rng.choice((mpx.MODE_PINGPONG, mpx.MODE_UNIDIR)), gpu_group=rng.randrange(2),
                         n=rng.choice(sizes), iters=rng.randrange(10), nwg=rng.choice(SOAK_WIDTHS),
                         check=rng.random() < 0.5, reseed=rng.choice(SOAK_GPU + SOAK_HOST)))
    return plan
