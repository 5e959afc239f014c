"""The host link at rank slots up to 63, with shared ends, between calls of
other kinds on the same GPU rank, and the two statements of
include/mpx_hostlink.h about the recorder and the GPU-side deadline (-m gpu).

A HostBox row is indexed by the GPU peer's rank (up to 63) and a rank counts
its links per peer rank (tx_seq[host_rank], up to index 63); one endpoint may
serve several GPU ranks in turn and one GPU rank several endpoints.  A GPU
rank's host-link calls share its scratch words, status line and token with
its pair, armed and fan calls.  Every expectation is host bytes
(tests/hostlink.py, LinkMap): the whole rx and tx of the ends, the guard state
of every rank that took no part, and after every call every counter of every
attached rank towards every rank number of the context.  Every wait is
bounded; wall time is asserted in the two deadline cases only.
"""
import threading
import time

import pytest

import mpx
import oracle_py
import payload
from hostlink import LinkMap

pytestmark = pytest.mark.gpu

T = mpx.hostlink_ll_max()
PP, UNI, NB = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR, mpx.MODE_NONBLOCKING
BIG = (256 << 10) + 21
WIDE = 16        # a width asked for; at 4161 B the 1 KiB-per-workgroup rule narrows it to 5


# ---- rows up to 63 ------------------------------------------------------------
# (rank 63 is an endpoint in one map and a GPU rank in the other: a rank number is one or the other)
@pytest.mark.parametrize("gpu,host,links", [([62, 5], [63, 40], [(62, 63), (5, 40)]), ([63, 9], [0, 31], [(63, 0)])],
                         ids=["62-63,5-40", "63-0"])
def test_rows_up_to_63(gpu, host, links):
    h = LinkMap(BIG, 64, gpu, host, links)
    try:
        for link in links:
            for mode in (PP, UNI):
                for gpu_group in (1, 0):
                    for n, nwg in ((8, 0), (T, 0), (4161, WIDE), (BIG, 7)):
                        out = h.call([link], mode, gpu_group, n, 5, nwg=nwg, what=("rows", link, mode, gpu_group, n))
                        assert all(t.nwg == {8: 1, T: 1, 4161: 5, BIG: 7}[n] for t in out.values())
        for g, e in links:
            assert h.counters(g, e)["tx_seq"] == h.counters(e, g)["rx_seq"] == 2 * 2 * 4 * 5
    finally:
        h.close()


# ---- one endpoint, several GPU ranks --------------------------------------------
SERVED = [1, 9, 33, 37]     # equal in their low 3 bits (1, 9, 33) or low 5 bits (1, 33)
EP = 20


def served_map(n):
    return LinkMap(n, 64, SERVED, [EP], [(g, EP) for g in SERVED])


@pytest.mark.parametrize("gpu_group", [1, 0], ids=["gpu_to_cpu", "cpu_to_gpu"])
def test_one_endpoint_after_gpu_ranks_that_would_alias_ll(gpu_group):
    """An end is in one call at a time, so a row index that lost its high bits
    shows only through what the earlier GPU rank LEFT in the shared row.  The
    LL wait wants its tag exactly: every link is moved to where its first
    message has the number of the previous link's last, and the sizes
    descend (T, 100, 8, 1), so the earlier message's units cover the new one.
    A receiver that reads the aliased row finds its tag there at once and
    takes the earlier sender's bytes, which differ: every GPU rank has its
    own tx seed, and the endpoint's tx is drawn anew for every link.  The
    sender enters 0.05 s late, so the row holds nothing but the past when the
    receiver looks.  gpu_group 1: unidir GPU -> CPU (in.ll); 0: CPU -> GPU
    (out.ll)."""
    h = served_map(T)
    try:
        last = None
        for k, (g, n) in enumerate(zip(SERVED, (T, 100, 8, 1))):
            link = (g, EP)
            h.set_tx(EP, 40 + k)
            if last is not None:
                h.jump(link, last)
            sender = g if gpu_group == 1 else EP
            h.call([link], UNI, gpu_group, n, 5, delay={sender: 0.05}, what=f"LL alias: sender {sender} of link {link}, {n} B")
            assert last is None or h.counters(g, EP)["tx_seq"] == last + 4
            last = h.counters(g, EP)["tx_seq"]
    finally:
        h.close()


def test_one_endpoint_after_gpu_ranks_that_would_alias_bulk():
    """The waits on flag, credit, ready and posted are "word >= expected", so
    the links stand at descending counts in the order they are used: a stale,
    higher word of the earlier GPU rank's row lets the receiver go on before
    its bytes landed (it then checksums the guard bytes).  Unidir in both
    directions with the sender 0.05 s late, then ping-pong."""
    n = 4161
    h = served_map(n)
    try:
        for k, g in enumerate(SERVED):
            h.advance((g, EP), seq_by=10000 * (4 - k), calls_by=100 * (4 - k))
        for gpu_group in (1, 0):
            for k, g in enumerate(SERVED):
                h.set_tx(EP, 60 + 4 * gpu_group + k)
                sender = g if gpu_group == 1 else EP
                h.call([(g, EP)], UNI, gpu_group, n, 5, nwg=WIDE, delay={sender: 0.05},
                       what=f"bulk alias: sender {sender} of link {(g, EP)}")
        for g in SERVED:
            for gpu_group in (1, 0):
                h.call([(g, EP)], PP, gpu_group, n, 5, nwg=WIDE, what=f"bulk alias, ping-pong: link {(g, EP)}")
        counts = [h.counters(EP, g) for g in SERVED]
        assert all(a["rx_seq"] > b["rx_seq"] + 5000 and a["calls"] > b["calls"] + 50 for a, b in zip(counts, counts[1:]))
    finally:
        h.close()


# ---- one GPU rank, two endpoints --------------------------------------------------
def test_one_gpu_rank_with_two_endpoints():
    """used alternately: each endpoint has its own mailbox and tx, the GPU
    rank counts per host rank"""
    h = LinkMap(4161, 3, [0], [1, 2], [(0, 1), (0, 2)])
    try:
        with pytest.raises(ValueError):
            h.run([(0, 1), (0, 2)], PP, 1, 8, 1)          # one rx cannot serve two calls at once
        steps = [(PP, 1, 4161, 5), (UNI, 0, 4161, 4), (PP, 0, 8, 3), (UNI, 1, T, 2), (PP, 1, T + 1, 6), (UNI, 0, 8, 7)]
        for k, (mode, gpu_group, n, iters) in enumerate(steps):
            for link in ((0, 1), (0, 2)) if k % 2 == 0 else ((0, 2), (0, 1)):
                h.call([link], mode, gpu_group, n, iters + link[1], nwg=WIDE, what=("two endpoints", k, link))
        assert h.counters(0, 1)["tx_seq"] == sum(s[3] + 1 for s in steps)
        assert h.counters(0, 2)["tx_seq"] == sum(s[3] + 2 for s in steps) == h.counters(2, 0)["rx_seq"]
    finally:
        h.close()


# ---- mixed calls on one GPU rank ----------------------------------------------------
def test_host_link_between_pair_armed_and_fan_calls():
    """GPU ranks 0 and 1, endpoints 2 and 3.  Rank 0 alternates host-link calls
    with a pair call, a fan call, an armed and started call and an armed and
    disarmed one: they share me.scratch (kScrLanded and words 0..3 are reset by
    finish_last, the relay words by the host-link kernel), the status line and
    the token.  Then rank 0 runs its host link while rank 1 is inside a
    non-blocking self-send."""
    n, stride = 4161, 4352
    h = LinkMap(2 * stride, 4, [0, 1], [2, 3], [(0, 2), (1, 3)])
    a = (0, 2)
    try:
        h.call([a], UNI, 0, n, 5, nwg=WIDE, what="1: host-link bulk unidir, the GPU pulls (kScrLanded)")
        h.pair(0, 1, PP, 8, 5, what="2: pair ping-pong LL")
        h.call([a], PP, 1, 8, 5, what="3: host-link LL")
        h.fan([0, 1], n, stride, 3, what="4: fan over {0, 1}")
        h.call([a], PP, 0, n, 5, nwg=WIDE, what="5: host-link bulk ping-pong")
        h.pair(0, 1, PP, n, 4, armed=True, what="6: armed and started pair call")
        h.call([a], UNI, 1, n, 5, nwg=WIDE, what="7: host-link unidir, the other way")

        def arm_and_disarm():
            h.reset_rx()
            exp, ack = h.expect(0, 1, n)
            h.c.arm(PP, 1, 0, 1, 3, *h.gpu[0], n, check_payload=True, expect=exp, expect_ack=ack, timeout_ms=5000)
            h.c.disarm(0)
            h.untouched((), "8: armed and disarmed")
        h.counted_moves({}, {0: 1}, arm_and_disarm, "8: armed and disarmed (the token is spent, the numbers come back)")
        h.call([a], PP, 0, 8, 5, what="9: host-link LL")
        h.call([(0, 2), (1, 3)], PP, 1, n, 5, nwg=WIDE, what="both links at once")

        # rank 0 on its host link while rank 1 is inside a non-blocking self-send
        iters_self = 2000
        was = h.all_counters()
        h.reset_rx()
        out, errs = h.run([a], PP, 1, n, 33, nwg=WIDE,
                          also=[lambda: h.c.xfer(NB, 0, 1, 1, iters_self, *h.gpu[1], n, timeout_ms=5000)])
        assert not errs, {k: str(e) for k, e in errs.items()}
        t1 = h.also_out[0]
        assert isinstance(t1, mpx.Timing), t1
        assert t1.recv_done == oracle_py.lib().oracle_nb_waited(iters_self)
        h.verify(out, [a], PP, 1, n, 33, True, "host link beside a self-send")
        payload.compare(h.rx(1), h.tx_bytes[1][:n] + h.blank()[n:], 0, "rank 1's rx after its self-send")
        payload.compare(h.rx(3), h.blank(), 0, "rx of endpoint 3, which took no part")
        now = h.all_counters()
        for (x, y), w in was.items():
            if (x, y) == (1, 1):
                continue                                   # (the self-send's own link)
            moved = 33 if (x, y) in ((0, 2), (2, 0)) else 0
            want = dict(tx_seq=w["tx_seq"] + moved, rx_seq=w["rx_seq"] + moved, calls=w["calls"] + (1 if moved else 0),
                        token=0 if x in h.host else w["token"] + (1 if x in (0, 1) else 0))
            assert now[x, y] == want, ((x, y), w, now[x, y], want)
    finally:
        h.close()


# ---- the recorder --------------------------------------------------------------------
def test_host_link_calls_are_never_traced():
    """"Host-link calls are never traced by the latency recorder": with the
    recorder on, a host-link call leaves the block exactly as it was; the
    pair ping-pong that follows is recorded with its own iteration count; a
    host-link call afterwards still delivers its bytes"""
    h = LinkMap(4161, 3, [0, 1], [2], [(0, 2)])
    try:
        h.c.lat_enable(0, 16)
        blank = h.c.lat_get(0)
        assert blank["calls"] == 0 and blank["count"] == 0
        for mode, gpu_group, n in ((PP, 1, 8), (PP, 0, 4161), (UNI, 1, 4161), (UNI, 0, 8)):
            h.call([(0, 2)], mode, gpu_group, n, 7, nwg=WIDE, what=("recorder on", mode, gpu_group, n))
            assert h.c.lat_get(0) == blank and h.c.lat_raw(0) == []
        h.pair(0, 1, PP, 8, 11, what="a traced pair call")
        got = h.c.lat_get(0)
        assert (got["calls"], got["last_iters"], got["count"]) == (1, 11, 11), got
        h.call([(0, 2)], PP, 1, 4161, 7, nwg=WIDE, what="after the traced call")
        assert h.c.lat_get(0) == got
        h.c.lat_disable(0)
        h.call([(0, 2)], PP, 0, 8, 3, what="recorder off")
    finally:
        h.close()


# ---- the GPU-side deadline -----------------------------------------------------------
@pytest.mark.parametrize("group", [1, 0])
def test_gpu_side_deadline(group):
    """"The GPU's waits are bounded by opts.timeout_ms on the kernel's clock":
    mpx_xfer_hostlink alone at 4161 B and five workgroups, timeout_ms = 300,
    the endpoint never calls.  Group 1: workgroup 0 runs out at the endpoint's
    `posted`, the other four at the relay word kScrHostPosted, which workgroup
    0 never writes.  Group 0: workgroup 0 runs out at `ready`, the others at
    kScrHostSeen.  MPX_ERR_TIMEOUT naming iteration 0 inside 5 s, then
    MPX_ERR_STATE; a fresh context in the same process works.

    Why every workgroup reaches last_to_finish after the abort (read in
    mpx_kernels.hip): each of these waits is Loop::poll_ge — thread 0 spins,
    and every 64 spins should_stop looks at its own LDS abort flag, at
    scratch word 1 (another workgroup's give_up) and at the kernel clock
    against timeout_ticks; whichever ends the spin, give_up sets the LDS flag,
    scratch word 1 and the status line, the workgroup meets at poll_ge's
    __syncthreads and poll_ge returns false.  The group-1 posted wait then
    leaves `ok` false and the loop body is never entered; in group 0 recv(0)
    returns false and the loop ends (`ok && i < iters`).  No wait lies between
    there and last_to_finish, whose only wait is workgroup 0's for the count
    of the other workgroups — each of which adds itself right after its own
    drain.  So the kernel ends at most one deadline (plus 64 spins) after the
    launch, whichever workgroup's clock runs out first."""
    n = 4161
    h = LinkMap(n, 2, [0], [1], [(0, 1)])
    try:
        got = {}

        def gpu_side(key):
            try:
                got[key] = h.c.xfer_hostlink(PP, group, 0, 1, 3, *h.gpu[0], n, timeout_ms=300, nwg=WIDE)
            except mpx.MpxError as e:
                got[key] = e
        for key in ("first", "second"):
            t0 = time.monotonic()
            th = threading.Thread(target=gpu_side, args=(key,), daemon=True)
            th.start()
            th.join(20.0)
            assert not th.is_alive(), "the GPU side is still inside its call 20 s after a 300 ms deadline"
            took = time.monotonic() - t0
            e = got[key]
            assert isinstance(e, mpx.MpxError), e
            if key == "first":
                assert e.status == mpx.ERR_TIMEOUT and "timed out at iteration 0" in str(e) and took < 5.0, (str(e), took)
            else:
                assert e.status == mpx.ERR_STATE, str(e)
        payload.compare(h.rx(1), h.blank(), 0, "the endpoint's rx: nothing was pushed")
    finally:
        h.close()
    h = LinkMap(n, 2, [0], [1], [(0, 1)])
    try:
        h.call([(0, 1)], PP, group, n, 3, nwg=WIDE, what="a fresh context after the deadline")
    finally:
        h.close()
