"""The host-link recorder (include/mpx_hostlink_lat.h) on loopback GPU 0: the
per-iteration latency distribution of the host link's ping-pong and unidir
loops, recorded on the GPU end (k_hostlink_lat, the kernel's 10 ns clock) and
on the CPU end (mpx_hostlink.h's traced loop, CLOCK_MONOTONIC nanoseconds).

Every call goes through LinkMap.call (tests/hostlink.py): both ends' rx and tx
byte for byte, what the call reported, every counter of every attached rank.
"""
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import hostlink_duplex
import mpx
from hostlink import LinkMap

pytestmark = pytest.mark.gpu

GT, HT = 1e-8, 1e-9            # tick_s of a GPU rank and of an endpoint
PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
STAT_KEYS = ("count", "calls", "min_ticks", "max_ticks", "sum_ticks", "max_iter", "last_iters")
G, H = 0, 1                     # the one-link maps: GPU rank 0, endpoint 1
N_MAX = 4161
# LL on both sides, the last LL size, the first bulk size, bulk at width 7 (the
# grid then has workgroups that do not trace); unidir mixes a bulk payload with an LL ack
SIZES = [(8, 0), (256, 0), (257, 0), (4161, 7)]


def bucket_counts(d):
    return np.bincount([mpx.lat_bucket(int(x)) for x in d], minlength=mpx.LAT_BUCKETS).tolist()


def deltas(raw):
    return [b - a for a, b in zip(raw, raw[1:])]


def tick_of(M, r):
    return GT if r in M.gpu else HT


def is_zero(lat, tick):
    return all(lat[k] == 0 for k in STAT_KEYS) and not any(lat["hist"]) and lat["tick_s"] == tick


def stats_equal_trace(lat, raw, iters, tick, what, calls=1):
    """one traced call, whole inside the raw trace: the block's streamed
    statistics are the trace's own, in integer ticks of that end's clock"""
    assert len(raw) == iters + 1, (what, len(raw))
    d = deltas(raw)
    assert all(x >= 0 for x in d), (what, "stamps decrease")
    assert lat["tick_s"] == tick, (what, lat["tick_s"])
    assert lat["count"] == iters and lat["calls"] == calls and lat["last_iters"] == iters, (what, lat)
    assert (lat["min_ticks"], lat["max_ticks"], lat["sum_ticks"]) == (min(d), max(d), sum(d)), (what, lat, d)
    assert lat["sum_ticks"] == raw[-1] - raw[0], what                # the sum telescopes
    assert lat["hist"] == bucket_counts(d), what
    assert lat["max_iter"] == int(np.argmax(d)), (what, lat["max_iter"], d)   # the first maximum


def snapshot(c, r, peer):
    return c.hostlink_lat_get(r, peer), c.hostlink_lat_raw(r, peer)


def status_of(call):
    with pytest.raises(mpx.MpxError) as e:
        call()
    return e.value.status


@pytest.fixture(scope="module")
def link():
    """GPU rank 0 and endpoint 1, one link; every test leaves both recorders off"""
    M = LinkMap(N_MAX, 2, [G], [H], [(G, H)])
    yield M
    M.close()


@pytest.fixture(autouse=True)
def recorders_off(request):
    yield
    if "link" in request.fixturenames:
        M = request.getfixturevalue("link")
        for r in (G, H):
            M.c.hostlink_lat_disable(r)


# ---- 1. streamed statistics equal the raw trace, on both ends ------------------------------
@pytest.mark.parametrize("n,nwg", SIZES)
@pytest.mark.parametrize("gpu_group", [1, 0])
@pytest.mark.parametrize("mode", [PP, UNI])
def test_streamed_statistics_equal_the_raw_trace(link, mode, gpu_group, n, nwg):
    M, c = link, link.c
    for r in (G, H):
        c.hostlink_lat_enable(r, 64)
    for iters in (1, 2, 33):
        for r in (G, H):
            c.hostlink_lat_reset(r)
        what = f"mode {mode} gpu_group {gpu_group} B {n} iters {iters}"
        M.call([(G, H)], mode, gpu_group, n, iters, check=True, nwg=nwg, what=what)
        ph = c.phases(G)
        for r, peer in ((G, H), (H, G)):
            lat, raw = snapshot(c, r, peer)
            stats_equal_trace(lat, raw, iters, tick_of(M, r), (what, r))
            d = deltas(raw)
            print(f"{what} rank {r}: min {min(d)} max {max(d)} sum {sum(d)} ticks of {lat['tick_s']:.0e} s")
        # the GPU end: t[0] is the instant first_iter_s counts from, t[1] the kTsFirst stamp itself
        d0 = deltas(c.hostlink_lat_raw(G, H))[0]
        assert abs(d0 * GT - ph["first_iter_s"]) < 0.5e-8, (what, d0, ph["first_iter_s"])
        assert c.hostlink_lat_get(H, G)["tick_s"] == 1e-9


# ---- 2. raw cap -------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [4, 0])
def test_raw_trace_is_capped_and_the_statistics_are_not(link, cap):
    M, c = link, link.c
    for r in (G, H):
        c.hostlink_lat_enable(r, cap)
    M.call([(G, H)], PP, 1, 257, 7, what=f"cap {cap}")
    for r, peer in ((G, H), (H, G)):
        lat, raw = snapshot(c, r, peer)
        assert len(raw) == (5 if cap else 0), (r, raw)               # t[0] alone says nothing: cap 0 reports none
        assert lat["count"] == 7 and lat["calls"] == 1 and lat["last_iters"] == 7 and sum(lat["hist"]) == 7
        assert 0 < lat["min_ticks"] <= lat["max_ticks"] <= lat["sum_ticks"] and lat["max_iter"] < 7
        if cap:
            d = deltas(raw)
            assert all(x >= 0 for x in d) and min(d) >= lat["min_ticks"] and max(d) <= lat["max_ticks"]
            assert sum(d) <= lat["sum_ticks"]


def test_a_call_without_iterations(link):
    M, c = link, link.c
    for r in (G, H):
        c.hostlink_lat_enable(r, 8)
    M.call([(G, H)], PP, 1, 4161, 5, what="five")
    before = {r: c.hostlink_lat_get(r, p) for r, p in ((G, H), (H, G))}
    M.call([(G, H)], PP, 1, 4161, 0, what="none")
    for r, peer in ((G, H), (H, G)):
        lat, raw = snapshot(c, r, peer)
        want = dict(before[r], calls=2, last_iters=0)
        assert lat == want, (r, lat, want)                            # one more call, nothing else
        assert len(raw) == 1                                          # t[0] of the empty call


# ---- 3. accumulate, reset, disable, enable again ------------------------------------------------
def test_accumulate_reset_disable(link):
    M, c = link, link.c
    ends = ((G, H), (H, G))
    for r in (G, H):
        c.hostlink_lat_enable(r, 4)
    M.call([(G, H)], PP, 1, 8, 10, what="first")
    first = {r: snapshot(c, r, p) for r, p in ends}
    assert all(len(first[r][1]) == 5 for r in (G, H))
    M.call([(G, H)], UNI, 0, 4161, 6, nwg=7, what="second")
    for r, p in ends:
        lat, raw = snapshot(c, r, p)
        a = first[r][0]
        assert lat["count"] == 16 and lat["calls"] == 2 and lat["last_iters"] == 6 and sum(lat["hist"]) == 16
        assert lat["min_ticks"] <= a["min_ticks"] and lat["max_ticks"] >= a["max_ticks"]
        assert lat["sum_ticks"] > a["sum_ticks"] and all(x >= y for x, y in zip(lat["hist"], a["hist"]))
        assert len(raw) == 5 and raw != first[r][1]                   # the last traced call's stamps
    for r, p in ends:
        c.hostlink_lat_reset(r)
        assert is_zero(c.hostlink_lat_get(r, p), tick_of(M, r)) and c.hostlink_lat_raw(r, p) == []
    M.call([(G, H)], PP, 0, 257, 3, what="after reset")
    assert all(c.hostlink_lat_get(r, p)["count"] == 3 for r, p in ends)
    # disabled: calls run untraced, reads are refused, and enabling again resets
    for r in (G, H):
        c.hostlink_lat_disable(r)
    M.call([(G, H)], PP, 0, 257, 3, what="disabled")
    for r, p in ends:
        assert status_of(lambda: c.hostlink_lat_get(r, p)) == mpx.ERR_STATE
        assert status_of(lambda: c.hostlink_lat_raw(r, p)) == mpx.ERR_STATE
        assert status_of(lambda: c.hostlink_lat_reset(r)) == mpx.ERR_STATE
    # a larger cap regrows the blocks and resets them
    for r in (G, H):
        c.hostlink_lat_enable(r, 600)
        assert is_zero(c.hostlink_lat_get(r, 1 - r), tick_of(M, r))
    M.call([(G, H)], PP, 1, 8, 500, what="regrown")
    for r, p in ends:
        stats_equal_trace(*snapshot(c, r, p), 500, tick_of(M, r), ("regrown", r))
    # a smaller one keeps the allocation and still bounds the trace
    for r in (G, H):
        c.hostlink_lat_enable(r, 2)
    M.call([(G, H)], PP, 1, 8, 9, what="smaller")
    for r, p in ends:
        lat, raw = snapshot(c, r, p)
        assert len(raw) == 3 and lat["count"] == 9 and lat["calls"] == 1


# ---- 4. keyed by the peer's rank ----------------------------------------------------------------
def test_blocks_are_keyed_by_the_peers_rank():
    """GPU rank 0 has the endpoints 5 and 63, endpoint 63 the GPU ranks 0 and
    62, in a 64-rank context: each link's block holds only its own calls"""
    links = [(0, 5), (0, 63), (62, 63)]
    M = LinkMap(N_MAX, 64, [0, 62], [5, 63], links)
    try:
        c = M.c
        for r in M.attached():
            c.hostlink_lat_enable(r, 16)
        plan = {(0, 5): (PP, 1, 8, 3), (0, 63): (UNI, 0, 4161, 4), (62, 63): (PP, 0, 257, 5)}
        for l, (mode, grp, n, iters) in plan.items():
            M.call([l], mode, grp, n, iters, what=f"link {l}")
        for (g, h), (mode, grp, n, iters) in plan.items():
            for r, p in ((g, h), (h, g)):
                stats_equal_trace(*snapshot(c, r, p), iters, tick_of(M, r), ("keyed", r, p))
        # a second call on one link moves that link's two blocks only
        before = {(r, p): snapshot(c, r, p) for g, h in links for r, p in ((g, h), (h, g))}
        M.call([(0, 63)], PP, 1, 8, 2, what="again")
        for (r, p), was in before.items():
            now = snapshot(c, r, p)
            if (r, p) in ((0, 63), (63, 0)):
                assert now[0]["calls"] == 2 and now[0]["count"] == was[0]["count"] + 2 and len(now[1]) == 3
            else:
                assert now == was, (r, p)
        # peers never used read zeros, with that end's tick
        for r, p in ((0, 62), (0, 1), (62, 5), (62, 0), (5, 62), (5, 63), (63, 5), (63, 1)):
            assert is_zero(c.hostlink_lat_get(r, p), tick_of(M, r)), (r, p)
            assert c.hostlink_lat_raw(r, p) == []
    finally:
        M.close()


# ---- 5. independence ----------------------------------------------------------------------------
def test_the_three_recorders_are_independent():
    M = LinkMap(N_MAX, 3, [0, 1], [2], [(0, 2)])
    try:
        c = M.c
        for r in (0, 1):
            c.lat_enable(r, 16)
            c.fan_lat_enable(r, 16)
        c.hostlink_lat_enable(0, 16)
        c.hostlink_lat_enable(2, 16)

        def others():
            return {r: (c.lat_get(r), c.lat_raw(r), c.fan_lat_get(r, 1 - r), c.fan_lat_raw(r, 1 - r)) for r in (0, 1)}

        def mine():
            return {(r, p): snapshot(c, r, p) for r, p in ((0, 2), (2, 0), (0, 1))}
        o0 = others()
        assert all(x[0]["calls"] == 0 and x[2]["calls"] == 0 for x in o0.values())
        # a host-link call moves only this recorder
        M.call([(0, 2)], PP, 1, 4161, 5, nwg=7, what="host link")
        assert others() == o0
        m1 = mine()
        assert m1[0, 2][0]["count"] == 5 and m1[2, 0][0]["count"] == 5 and is_zero(m1[0, 1][0], GT)
        # a pair ping-pong moves only mpx_lat
        M.pair(0, 1, PP, 8, 6, what="pair")
        assert mine() == m1
        o1 = others()
        for r in (0, 1):
            assert o1[r][0]["count"] == 6 and o1[r][0]["calls"] == 1 and len(o1[r][1]) == 7
            assert o1[r][2:] == o0[r][2:]
        # a full-duplex call moves none
        hostlink_duplex.call(M, [(0, 2)], 4161, 5, what="duplex")
        assert mine() == m1 and others() == o1
    finally:
        M.close()


@pytest.mark.parametrize("traced", [G, H])
def test_one_end_traced(link, traced):
    """tracing is local: the same bytes (LinkMap.call verifies them), the
    traced end's block filled, the untraced end's reads refused"""
    M, c = link, link.c
    other = 1 - traced
    c.hostlink_lat_enable(traced, 16)
    for mode, grp, n in ((PP, 1, 8), (UNI, 0, 4161)):
        c.hostlink_lat_reset(traced)
        M.call([(G, H)], mode, grp, n, 6, what=f"only rank {traced} traced")
        stats_equal_trace(*snapshot(c, traced, other), 6, tick_of(M, traced), ("one end", traced))
        assert status_of(lambda: c.hostlink_lat_get(other, traced)) == mpx.ERR_STATE


# ---- 6. statuses --------------------------------------------------------------------------------
def test_other_engines_refuse_the_host_link_recorder():
    with mpx.Context(2, "sdma") as c:
        assert status_of(lambda: c.hostlink_lat_enable(0, 16)) == mpx.ERR_UNSUPPORTED


def test_statuses():
    M = LinkMap(8, 5, [0, 1], [2], [(0, 2)])                         # ranks 3 and 4: never attached
    try:
        c = M.c
        five = lambda r, p: (lambda: c.hostlink_lat_enable(r, 16), lambda: c.hostlink_lat_disable(r),   # noqa: E731
                             lambda: c.hostlink_lat_reset(r), lambda: c.hostlink_lat_get(r, p),
                             lambda: c.hostlink_lat_raw(r, p))
        for r in (3, 5, -1):                                         # neither a local GPU rank nor an endpoint
            for call in five(r, 0):
                assert status_of(call) == mpx.ERR_INVALID
        for r in (0, 2):
            for cap in (-1, mpx.HOSTLINK_LAT_RAW_MAX + 1):
                assert status_of(lambda: c.hostlink_lat_enable(r, cap)) == mpx.ERR_INVALID
            for call in five(r, 2 - r)[2:]:                          # not enabled
                assert status_of(call) == mpx.ERR_STATE
            c.hostlink_lat_disable(r)                                # (disable of a disabled recorder: fine)
            c.hostlink_lat_enable(r, 0)
            c.hostlink_lat_enable(r, 16)
            for peer in (r, 5, -1):
                assert status_of(lambda: c.hostlink_lat_get(r, peer)) == mpx.ERR_INVALID
                assert status_of(lambda: c.hostlink_lat_raw(r, peer)) == mpx.ERR_INVALID
            n = mpx.C.c_int(0)
            assert c.L.mpx_hostlink_lat_get(c.h, r, 2 - r, None) == mpx.ERR_INVALID
            assert c.L.mpx_hostlink_lat_raw(c.h, r, 2 - r, None, 4, mpx.C.byref(n)) == mpx.ERR_INVALID
            assert c.L.mpx_hostlink_lat_raw(c.h, r, 2 - r, None, 0, None) == mpx.ERR_INVALID
            assert is_zero(c.hostlink_lat_get(r, 4), tick_of(M, r))   # in range, never used: zeros
        # mpx_lat_enable on an endpoint is what it was
        assert status_of(lambda: c.lat_enable(2, 16)) == mpx.ERR_STATE
        # a GPU rank that holds an armed call refuses all five; the endpoint's are not concerned
        exp, ack = M.expect(0, 1, 8)
        c.arm(PP, 1, 0, 1, 3, *M.gpu[0], 8, check_payload=True, expect=exp, expect_ack=ack, timeout_ms=5000)
        try:
            for call in five(0, 2):
                assert status_of(call) == mpx.ERR_STATE
            c.hostlink_lat_reset(2)
            assert is_zero(c.hostlink_lat_get(2, 0), HT)
        finally:
            c.disarm(0)
        M.call([(0, 2)], PP, 1, 8, 4, what="after the disarm")
        stats_equal_trace(*snapshot(c, 0, 2), 4, GT, "after the disarm")
    finally:
        M.close()


# ---- 7. a stalled iteration is found at its index, on both ends ---------------------------------
LAG_US = 20000


@pytest.mark.parametrize("n,nwg", [(8, 0), (4161, 7)])
@pytest.mark.parametrize("gpu_group", [1, 0])
@pytest.mark.parametrize("mode", [PP, UNI])
def test_a_stalled_iteration_is_found_at_its_index_on_both_ends(link, monkeypatch, mode, gpu_group, n, nwg):
    """positive control: the endpoint busy-waits 20 ms before its first step of
    iteration 10 of 20 (MPX_TEST host_lag).  Both ends see that iteration, and
    only it, take the 20 ms: the endpoint itself, and the GPU rank, whose
    iteration 10 cannot end before the endpoint's send of iteration 10.  The
    thresholds come from the injected value; iteration 0 is excluded, it may
    hold the wait for the peer's entry.

    Measured on MI355X boxes, four runs of the eight cases: the endpoint's
    longest iteration was 20.0004 to 20.0129 ms, and the GPU rank's followed
    it to within -1.0 .. +0.7 us (the two clocks agreed to 3e-5 over the 2000
    iterations of test_the_two_clocks_see_the_same_loop).  Seven cases passed
    every time, the GPU rank at 20.0005 to 20.0135 ms.  The eighth, ping-pong
    at 8 B with the GPU rank as group 1, MISSED THE 20 ms BOUND ON THE GPU END
    in two of the four runs: 19.99912 ms, and 19.99936 ms where the endpoint
    read 20.00038 ms; in the other two (inside the whole suite) it passed.  There
    the endpoint's iteration is the stall plus 0.4 us
    (its receive is already in, its LL send is one store), and the GPU rank's
    two stamps around it each lie one poll across the link behind the
    endpoint's sends; a poll is a link round trip of about 1.1 us, and after
    20 ms of polling its phase is no longer the steady state's.  The bound is
    the issue's and stays; max_iter and the other deltas hold in every case."""
    M, c = link, link.c
    for r in (G, H):
        c.hostlink_lat_enable(r, 32)
    monkeypatch.setenv("MPX_TEST", f"host_lag=10:{LAG_US}")
    M.call([(G, H)], mode, gpu_group, n, 20, nwg=nwg, what="lagged")
    monkeypatch.setenv("MPX_TEST", "")
    longest = {}
    for r, peer in ((H, G), (G, H)):
        lat, raw = snapshot(c, r, peer)
        tick = tick_of(M, r)
        d = deltas(raw)
        longest[r] = lat["max_ticks"] * tick
        print(f"rank {r}: max {longest[r] * 1e3:.5f} ms at iteration {lat['max_iter']}; "
              f"others up to {max(x for i, x in enumerate(d) if i not in (0, 10)) * tick * 1e6:.1f} us, d[0] {d[0] * tick * 1e6:.1f} us")
        stats_equal_trace(lat, raw, 20, tick, ("lagged", r))
        assert lat["max_iter"] == 10
        assert all(x * tick < LAG_US * 0.5e-6 for i, x in enumerate(d) if i >= 1 and i != 10), d
    print(f"GPU rank's longest over the endpoint's: {longest[G] / longest[H]:.6f}")
    assert longest[H] >= LAG_US * 1e-6
    assert longest[G] >= LAG_US * 1e-6


# ---- 8. the two clocks see the same loop --------------------------------------------------------
def test_the_two_clocks_see_the_same_loop(link):
    """one 8-byte ping-pong of 2000 iterations, both ends traced whole: the
    span t[1] .. t[2000] by the endpoint's clock (ns) over the GPU rank's
    (10 ns ticks) lies in [0.98, 1 / 0.98], the bound the kernel clock is held
    to against the host clock (tests/test_gpu_lat.py).  The two windows differ
    by at most one iteration at each edge (0.1 %); a wrong tick_s on either
    end is off by a factor of 10."""
    M, c = link, link.c
    iters = 2000
    for r in (G, H):
        c.hostlink_lat_enable(r, 2048)
    M.call([(G, H)], PP, 1, 8, iters, check=False, what="clocks")
    span = {}
    for r, peer in ((G, H), (H, G)):
        lat, raw = snapshot(c, r, peer)
        assert len(raw) == iters + 1
        span[r] = (raw[iters] - raw[1]) * lat["tick_s"]
    ratio = span[H] / span[G]
    print(f"endpoint {span[H] * 1e3:.4f} ms, GPU rank {span[G] * 1e3:.4f} ms, ratio {ratio:.5f}")
    assert 0.98 <= ratio <= 1 / 0.98, (span, ratio)


# ---- 9. mpx_perf -H -T --------------------------------------------------------------------------
LAT_HEADER = ("Timestamp,JobId,Rank,PeerRank,Mode,BufferSize,NumOfBuffers,RunId,Count,MinUs,P50Us,P90Us,P99Us,P999Us,"
              "MaxUs,MeanUs,MaxIter")


@pytest.mark.parametrize("args,h,n,proto", [(["-H", "1", "-b", "4161", "-c", "1"], "1", 4161, 12),
                                            (["-H", "2", "-u", "1", "-b", "8"], "2", 8, 11)])
def test_mpx_perf_writes_one_line_per_end(tmp_path, args, h, n, proto):
    from test_gpu_host import run
    p, recs, side = run(tmp_path, args + ["-T", "16", "-w", "1", "-f", "@G1", "-n", "1", "-p", "1", "-i", "7", "-r", "3",
                                          "-l", "@LOGS"], gpus="0")
    assert p.returncode == 0, p.stderr[-800:]
    assert len(recs) == 2 and len(side) == 2                         # the records are what they are without -T
    writer = 0 if h == "1" else 1
    files = glob.glob(str(tmp_path / "logs" / "lat-*.csv"))
    assert len(files) == 1
    name = os.path.basename(files[0])
    m = re.fullmatch(r"lat-([0-9a-f-]{36})-(\d)-\d{4}-\d\d-\d\d-\d\d-\d\d-\d\d\.csv", name)
    assert m and int(m.group(2)) == writer, name
    assert not fnmatch.fnmatch(name, "tcp*") and not fnmatch.fnmatch(name, "gpu-*.csv")
    lines = open(files[0]).read().splitlines()
    assert lines[0] == LAT_HEADER
    rows = [dict(zip(LAT_HEADER.split(","), x.split(","))) for x in lines[1:]]
    assert sorted((int(x["RunId"]), int(x["Rank"]), int(x["PeerRank"])) for x in rows) == \
        [(1, 0, 1), (1, 1, 0), (2, 0, 1), (2, 1, 0)]                  # one line per recorded run and end
    for x in rows:
        assert x["JobId"] == m.group(1) and int(x["Mode"]) == proto
        assert (int(x["BufferSize"]), int(x["NumOfBuffers"]), int(x["Count"])) == (n, 7, 7)
        mn, p50, mx = float(x["MinUs"]), float(x["P50Us"]), float(x["MaxUs"])
        assert 0 < mn <= p50 <= mx and 0 <= int(x["MaxIter"]) < 7
