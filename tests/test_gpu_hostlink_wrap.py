"""The host link across push 2^31, push 2^32, call 2^32 and token 2^32 (-m gpu).

The CPU endpoint restates every compare of the protocol in plain C++
(mpi-perf_amd/csrc/mpx_hostlink.h: ll_tag, the tag equality of recv_ll, the
`>= seq` waits of recv_bulk / send_bulk / posted); the kernel has its own.
mpx_test_advance_link (both ends of a link alike, a host endpoint included)
puts a link just short of such a point, and the calls then run across it.
"Near P": the link's next push is number P - 4.  A link jumps only before its
first LL message, so no LL message follows a larger one by a multiple of 2^31
pushes (the LL zone's documented alias) — every case gets a
fresh link: an endpoint of its own, whose mailbox no other case has touched.

Every expectation is host bytes (tests/hostlink.py, LinkMap): the whole rx and
tx of both ends after every call, the oracle's checksums, and every counter of
every attached rank (counted).  Every wait is bounded (timeout_ms = 5000, the
join limit); no time is asserted.
"""
import pytest

import mpx
import payload
from hostlink import P31, P32, LinkMap

pytestmark = pytest.mark.gpu

T = mpx.hostlink_ll_max()
PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
BOUNDARIES = [P31, P32]
MODES = [PP, UNI]
GROUPS = [1, 0]          # the GPU rank's group: 1 = it sends first (unidir: it sends the payload)


def one_gpu(n: int, nlinks: int) -> LinkMap:
    """GPU rank 0 with `nlinks` endpoints 1.., each a link of its own"""
    return LinkMap(n, 1 + nlinks, [0], range(1, 1 + nlinks), [(0, k) for k in range(1, 1 + nlinks)])


def across(h: LinkMap, link, P, mode, gpu_group, n, what, **kw):
    """the boundary inside one call: 9 iterations from near P"""
    h.jump(link, P - 4)
    h.call([link], mode, gpu_group, n, 9, what=(what, "inside"), **kw)
    assert h.counters(*link)["tx_seq"] == P + 4 == h.counters(link[1], link[0])["rx_seq"]


def between(h: LinkMap, link, P, mode, gpu_group, n, what, **kw):
    """the boundary between two calls: the first ends on push P - 1"""
    h.jump(link, P - 4)
    h.call([link], mode, gpu_group, n, 4, what=(what, "first of two"), **kw)
    assert h.counters(*link)["tx_seq"] == P - 1
    h.call([link], mode, gpu_group, n, 4, what=(what, "second of two"), **kw)
    assert h.counters(*link)["tx_seq"] == P + 3 == h.counters(link[1], link[0])["rx_seq"]


@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_ll_messages_across(P, mode, gpu_group):
    """0, 1, 8 and T bytes, all checked: ll_tag and the tag equality on both
    sides (the kernel's wait_ll, the endpoint's recv_ll)"""
    sizes = [0, 1, 8, T]
    h = one_gpu(T, 2 * len(sizes))
    try:
        for k, n in enumerate(sizes):
            across(h, h.links[2 * k], P, mode, gpu_group, n, ("ll", P, mode, gpu_group, n))
            between(h, h.links[2 * k + 1], P, mode, gpu_group, n, ("ll", P, mode, gpu_group, n))
    finally:
        h.close()


@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_ll_zone_history_across(monkeypatch, P, mode, gpu_group):
    """MPX_HOSTLINK_LL=8192 (read at every call): the whole 8 KiB row written
    just below P — in.ll and out.ll both (unidir: the payload's row; the other
    carries the ack) — then nine 8-byte messages across P, which rewrite only
    the first unit, then the whole row again: units 1.. still carry the tags of
    pushes P - 6 and P - 5 and must not be taken for the new ones.  Both ends'
    tx are rewritten between the calls, so a unit accepted on its old tag
    delivers old bytes."""
    monkeypatch.setenv("MPX_HOSTLINK_LL", "8192")
    assert mpx.hostlink_ll_max() == 8192
    h = one_gpu(8192, 1)
    link = h.links[0]
    try:
        h.jump(link, P - 6)
        for k, (n, iters) in enumerate(((8192, 2), (8, 9), (8192, 3))):
            for r in link:
                h.set_tx(r, 100 + k)
            out = h.call([link], mode, gpu_group, n, iters, what=("ll zone", P, mode, gpu_group, n))
            assert all(t.protocol == mpx.PROTO_HOSTLINK_LL and t.nwg == 1 for t in out.values())
        assert h.counters(*link)["tx_seq"] == P + 7
    finally:
        h.close()


@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_bulk_messages_across(P, mode, gpu_group):
    """4161 B at the default width (one workgroup: no relay) and at five
    workgroups, 71681 B at width 70 (an empty chunk), checked: flag[w],
    credit[w] and ready on both sides' compares, the relay words beside them;
    in unidir the 1-byte LL ack crosses P together with the payload"""
    assert payload.chunk_shape(70, 71681) == (70, 1040, 1, 68, 961)
    shapes = ((4161, 0, 1), (4161, 16, 5), (71681, 70, 70))     # (n, width asked for, width run)
    h = one_gpu(71681, 2 * len(shapes))
    try:
        for k, (n, nwg, width) in enumerate(shapes):
            for form, link in ((across, h.links[2 * k]), (between, h.links[2 * k + 1])):
                form(h, link, P, mode, gpu_group, n, ("bulk", P, mode, gpu_group, n, nwg), nwg=nwg)
            out = h.call([h.links[2 * k]], mode, gpu_group, n, 1, nwg=nwg)
            assert all(t.nwg == width and t.protocol == mpx.PROTO_HOSTLINK_BULK for t in out.values())
    finally:
        h.close()


@pytest.mark.parametrize("late", ["gpu", "host"])
@pytest.mark.parametrize("n", [8, 4161])
def test_a_compare_that_passes_early_is_seen(n, late):
    """P = 2^32, two ping-pong calls: the first ends on push P - 1, the second
    starts at push P and its first sender (group 1) enters 0.2 s late.  The
    receiver, in check mode on an rx reset to 0xEE, waits for push P all that
    time with the words of push P - 1 in front of it: a compare that lets the
    old word pass (0xffffffff >= 0 in 32 bits) checksums guard bytes and
    fails, and answers into the late side's rx, which is read the moment
    before that side enters and must still hold the guard state."""
    h = one_gpu(4161, 1)
    link = g, e = h.links[0]
    late_rank = g if late == "gpu" else e
    gpu_group = 1 if late == "gpu" else 0          # the late side sends first
    try:
        h.jump(link, P32 - 4)
        h.call([link], PP, gpu_group, n, 4, what=("early", n, late, "call 1"))
        assert h.counters(g, e)["tx_seq"] == P32 - 1

        def second():
            h.reset_rx()
            out, errs = h.run([link], PP, gpu_group, n, 1, check=True, delay={late_rank: 0.2},
                              before={late_rank: lambda: h.rx(late_rank)})
            assert not errs, {k: str(x) for k, x in errs.items()}
            payload.compare(h.seen[late_rank], h.blank(), 0, f"the late {late} side's rx before it entered")
            h.verify(out, [link], PP, gpu_group, n, 1, True, ("early", n, late, "call 2"))
            return out
        h.counted([link], 1, second, ("early", n, late))
        assert h.counters(g, e)["tx_seq"] == P32 == h.counters(e, g)["rx_seq"]
    finally:
        h.close()


@pytest.mark.parametrize("late", ["gpu", "host"])
def test_call_number_across_2_to_32(late):
    """calls = 2^32 - 2 on both ends, then call 2^32 - 1, a call without
    iterations (it posts nothing and takes no number), call 2^32 — whose first
    sender is on time and whose receiver enters 0.2 s late: nothing may land
    in the receiver's rx before it has posted call 2^32 (posted holds 2^32 - 1,
    which passes a 32-bit compare with 0) — and call 2^32 + 1."""
    n = 4161
    h = one_gpu(n, 1)
    link = g, e = h.links[0]
    late_rank = g if late == "gpu" else e
    gpu_group = 0 if late == "gpu" else 1          # the side that is on time sends first
    try:
        h.advance(link, calls_by=P32 - 2)
        assert h.counters(g, e)["calls"] == h.counters(e, g)["calls"] == P32 - 2
        h.call([link], PP, gpu_group, n, 3, what=("calls", late, 1))
        assert h.counters(g, e)["calls"] == P32 - 1
        h.call([link], PP, gpu_group, n, 0, what=("calls", late, "no iterations"))
        assert h.counters(g, e)["calls"] == h.counters(e, g)["calls"] == P32 - 1

        def second():
            h.reset_rx()
            out, errs = h.run([link], PP, gpu_group, n, 2, check=True, delay={late_rank: 0.2},
                              before={late_rank: lambda: h.rx(late_rank)})
            assert not errs, {k: str(x) for k, x in errs.items()}
            payload.compare(h.seen[late_rank], h.blank(), 0, f"the late {late} receiver's rx before it entered call 2^32")
            h.verify(out, [link], PP, gpu_group, n, 2, True, ("calls", late, 2))
            return out
        h.counted([link], 2, second, ("calls", late))
        assert h.counters(g, e)["calls"] == h.counters(e, g)["calls"] == P32
        h.call([link], UNI, 1 - gpu_group, 8, 3, what=("calls", late, 3))
        assert h.counters(g, e)["calls"] == P32 + 1
    finally:
        h.close()


def test_token_across_2_to_32():
    """the GPU rank's token at 2^32 - 2, then three host-link calls: the token
    of the second is 2^32, whose low half reads 0 in fin_word like the cleared
    status line"""
    h = one_gpu(4161, 1)
    link = g, e = h.links[0]
    try:
        h.advance_token(g, P32 - 2)
        assert h.counters(g, e)["token"] == P32 - 2 and h.counters(e, g)["token"] == 0
        for k, (mode, gpu_group, n, iters) in enumerate(((PP, 1, 4161, 5), (UNI, 0, 4161, 3), (PP, 0, 8, 4))):
            h.call([link], mode, gpu_group, n, iters, what=("token", k))
            assert h.counters(g, e)["token"] == P32 - 1 + k
    finally:
        h.close()


def test_hand_over_near_2_to_32():
    """one link near 2^32: host-link bulk, LL, unidir, and between them the GPU
    rank makes a checked pair call with another GPU rank on the same tx / rx;
    every counter of all three ranks is asserted after each step"""
    h = LinkMap(4161, 3, [0, 1], [2], [(0, 2)])
    link = (0, 2)
    try:
        h.jump(link, P32 - 4)
        h.call([link], PP, 1, 4161, 3, what="hand-over: bulk")                  # pushes P - 4 .. P - 2
        h.pair(0, 1, PP, 4161, 3, what="hand-over: pair bulk")
        h.call([link], PP, 0, 8, 3, what="hand-over: LL")                       # P - 1 .. P + 1
        h.pair(1, 0, UNI, 8, 2, what="hand-over: pair LL unidir")
        h.call([link], UNI, 1, 4161, 3, what="hand-over: unidir")
        h.pair(0, 1, PP, 2045, 2, what="hand-over: pair LL")
        h.call([link], UNI, 0, 4161, 2, what="hand-over: unidir, the other way")
        assert h.counters(0, 2)["tx_seq"] == h.counters(2, 0)["rx_seq"] == P32 - 5 + 11
        assert h.counters(0, 1)["tx_seq"] == h.counters(1, 0)["tx_seq"] == 7
    finally:
        h.close()
