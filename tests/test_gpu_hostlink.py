"""The host link on the GPU (include/mpx_hostlink.h): a GPU rank exchanges with
a CPU endpoint across the PCIe link, ping-pong and unidir, in both
orientations.  One GPU.  Every expectation is host bytes (tests/hostlink.py:
oracle_py.fill seeds tx, oracle_py.checksum sums it), never the library's own
output.  Buffers are attached 4 KiB longer than the message and rx starts as
0xEE, so every case also shows that no byte past the received range changed.
No time is asserted anywhere; every wait of every case is bounded (timeout_ms
<= 5000, and the helper's join limit).
"""
import json
import os
import re
import subprocess
import sys
import time

import pytest

import mpx
import payload
from hostlink import GUARD_BYTE, HostLinks

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T = mpx.hostlink_ll_max()
BIG = (256 << 10) + 21
PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
MASK = (1 << 64) - 1

_links = {}


def links(n: int, npairs: int = 1) -> HostLinks:
    """the links built for messages of n bytes, shared by the cases of that size"""
    key = (n, npairs)
    if key not in _links:
        _links[key] = HostLinks(n, npairs)
    _links[key].reset_rx()
    return _links[key]


def drop(n: int, npairs: int = 1) -> None:
    h = _links.pop((n, npairs), None)
    if h is not None:
        h.close()


@pytest.fixture(scope="module", autouse=True)
def _close_links():
    yield
    for key in list(_links):
        drop(*key)


def run_ok(h: HostLinks, n: int, *args, **kw):
    """a call that must succeed on every side; a link that failed is not reused"""
    try:
        out, errs = h.run(*args, **kw)
    except AssertionError:
        _links.pop((n, h.np), None)   # (a side still runs: the context is left alone)
        raise
    if errs:
        drop(n, h.np)
    assert not errs, {r: str(e) for r, e in errs.items()}
    return out


def assert_call(h: HostLinks, out, mode, gpu_group, n, iters, check):
    for r, t in out.items():
        gpu_side = r < h.np
        group = gpu_group if gpu_side else 1 - gpu_group
        what = f"rank {r} ({'GPU' if gpu_side else 'host'}, group {group}) mode {mode} n {n} iters {iters}"
        payload.compare(h.rx(r), h.want_rx(r, mode, group, n, iters), 0, what)
        assert t.recv_done == iters, what
        assert t.bytes == n * iters * (1 if mode == UNI else 2), what
        assert t.launches == (1 if gpu_side else 0), what
        assert t.protocol == (mpx.PROTO_HOSTLINK_LL if n <= T else mpx.PROTO_HOSTLINK_BULK), what
        if check:
            exp, ack = h.expect(r, n)
            want = ack if (mode == UNI and group == 1) else exp
            assert t.check_failures == 0 and t.check_iters == iters, what
            assert t.recv_digest == (want * iters) & MASK, what
        else:
            assert t.check_iters == 0 and t.recv_digest == 0, what


SIZES = [0, 1, 8, 2045, T, T + 1, 4161, BIG]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gpu_group", [1, 0])
@pytest.mark.parametrize("mode", [PP, UNI])
def test_bytes_no_check(mode, gpu_group, n, iters):
    h = links(n)
    out = run_ok(h, n, mode, gpu_group, n, iters)
    assert_call(h, out, mode, gpu_group, n, iters, False)


@pytest.mark.parametrize("n", [8, 2045, T + 1, 4161, BIG])
@pytest.mark.parametrize("gpu_group", [1, 0])
@pytest.mark.parametrize("mode", [PP, UNI])
def test_check_mode(mode, gpu_group, n):
    h = links(n)
    out = run_ok(h, n, mode, gpu_group, n, 33, check=True)
    assert_call(h, out, mode, gpu_group, n, 33, True)


@pytest.mark.parametrize("nwg,n", [(7, BIG), (70, 71681)])
@pytest.mark.parametrize("gpu_group", [1, 0])
@pytest.mark.parametrize("mode", [PP, UNI])
def test_ragged_widths(mode, gpu_group, nwg, n):
    """explicit widths whose chunks are ragged; 70 at 71681 B has an empty chunk"""
    width, chunk, empty, last, tail = payload.chunk_shape(nwg, n)
    assert width == nwg and (empty == 1 if nwg == 70 else n % chunk != 0)
    h = links(n)
    out = run_ok(h, n, mode, gpu_group, n, 5, check=True, nwg=nwg)
    assert_call(h, out, mode, gpu_group, n, 5, True)
    assert all(t.nwg == nwg for t in out.values())


def test_one_link_many_calls():
    """LL, bulk, LL, unidir each way (bulk payloads with LL acks, then an LL
    payload), ping-pong on ONE link: after every call both ends' counters have
    moved by that call's iterations and by one call.  The third step is the
    issue's "LL 2045 B" as min(2045, T) bytes: the measured threshold T is 256
    (DESIGN.md §5 "Host link"), where 2045 B would be a bulk message and the
    LL -> bulk -> LL alternation on the link's LL rows would be lost."""
    n_max = 4161
    h = links(n_max)
    g, e = 0, 1

    def counters():
        return h.c.link_counters(g, e), h.c.link_counters(e, g)

    was = counters()
    assert was[1]["token"] == 0
    assert T >= 8
    steps = [(PP, 1, 8, 5), (PP, 1, 4161, 4), (PP, 0, min(2045, T), 3),       # LL, bulk, LL again
             (UNI, 1, 4161, 6), (UNI, 0, 4161, 2), (UNI, 0, 8, 3),            # unidir each way; the last one LL
             (PP, 0, 4161, 7)]
    assert len(steps) == 7 and [s[0] for s in steps].count(UNI) == 3
    assert all((n <= T) == ll for (_, _, n, _), ll in zip(steps, (True, False, True, False, False, True, False)))
    for mode, gpu_group, n, iters in steps:
        h.reset_rx()
        out = run_ok(h, n_max, mode, gpu_group, n, iters, check=True)
        assert_call(h, out, mode, gpu_group, n, iters, True)
        now = counters()
        for end in (0, 1):
            for k in ("tx_seq", "rx_seq"):
                assert now[end][k] == was[end][k] + iters, (mode, n, end, k)
            assert now[end]["calls"] == was[end]["calls"] + 1, (mode, n, end)
        assert now[0]["token"] == was[0]["token"] + 1 and now[1]["token"] == 0
        was = now
    # a call that moves nothing: no counter but the GPU rank's token moves, both rx untouched
    h.reset_rx()
    out = run_ok(h, n_max, PP, 1, 4161, 0, check=True)
    assert_call(h, out, PP, 1, 4161, 0, True)
    now = counters()
    for end in (0, 1):
        assert {k: now[end][k] for k in ("tx_seq", "rx_seq", "calls")} == {k: was[end][k] for k in ("tx_seq", "rx_seq", "calls")}
    # and the link goes on
    out = run_ok(h, n_max, PP, 0, 8, 2, check=True)
    assert_call(h, out, PP, 0, 8, 2, True)


@pytest.mark.parametrize("late", ["host", "gpu"])
def test_a_payload_of_call_2_waits_for_its_receiver(late):
    """Call 1 moves 2045 B, call 2 4161 B.  One side enters call 2 0.2 s late;
    read the moment before it enters, its rx still holds call 1's payload and
    guards, although the other side — which sends first in call 2 — has been
    in call 2 all along."""
    n1, n2 = 2045, 4161
    h = links(n2)
    g, e = 0, 1
    late_rank = e if late == "host" else g
    gpu_group2 = 1 if late == "host" else 0          # the side that is on time sends first
    out = run_ok(h, n2, PP, gpu_group2, n1, 1)
    assert_call(h, out, PP, gpu_group2, n1, 1, False)
    late_group = (1 - gpu_group2) if late == "host" else gpu_group2
    held = h.want_rx(late_rank, PP, late_group, n1, 1)
    out = run_ok(h, n2, PP, gpu_group2, n2, 1, delay={late_rank: 0.2}, before={late_rank: lambda: h.rx(late_rank)})
    payload.compare(h.seen[late_rank], held, 0, f"the late {late} side's rx before it entered call 2")
    for r in (g, e):
        grp = gpu_group2 if r == g else 1 - gpu_group2
        payload.compare(h.rx(r), h.want_rx(r, PP, grp, n2, 1), 0, f"rank {r} after call 2")


@pytest.mark.parametrize("n", [4161, BIG])
def test_two_pairs_at_once(n):
    """GPU ranks 0 and 1 on GPU 0, host endpoints 2 and 3, four threads: each
    rank's tx has a seed of its own, so a byte of the other pair would show"""
    h = links(n, npairs=2)
    for mode, gpu_group in ((PP, 1), (UNI, 0)):
        h.reset_rx()
        out = run_ok(h, n, mode, gpu_group, n, 33, check=True)
        assert sorted(out) == [0, 1, 2, 3]
        assert_call(h, out, mode, gpu_group, n, 33, True)


@pytest.mark.parametrize("direction,n", [("d2h", 8), ("d2h", 4161), ("h2d", 8), ("h2d", 4161)])
def test_a_lost_payload_fails_the_receivers_check(direction, n):
    """MPX_TEST=skip_push=2 in a process of its own: the 2nd payload of a
    unidir call is lost on its way (LL: the tags arrive without the data;
    bulk: the flags / the pull without the stores).  The receiver returns
    MPX_ERR_CHECK with one failure, the sender MPX_OK, nothing times out."""
    env = dict(os.environ, MPX_TEST="skip_push=2")
    env.pop("MPX_HOSTLINK_LL", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "hostlink_worker.py"), direction, str(n)], capture_output=True,
                       text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["receiver"] == {"status": mpx.ERR_CHECK, "check_failures": 1, "check_iters": 5, "recv_done": 5}, got
    assert got["sender"] == {"status": mpx.OK, "check_failures": 0, "check_iters": 5, "recv_done": 5}, got
    # the control: the same call without the check passes unseen
    assert got["unchecked"] == [mpx.OK, mpx.OK], got


def test_cpu_side_deadline():
    """mpx_host_xfer alone (no kernel is launched): MPX_ERR_TIMEOUT within two
    seconds, the endpoint then refuses (MPX_ERR_STATE); a fresh context works"""
    n = 4161
    for group in (1, 0):
        h = HostLinks(n)
        try:
            t0 = time.monotonic()
            with pytest.raises(mpx.MpxError) as ei:
                h.c.host_xfer(PP, group, 1, 0, 3, n, timeout_ms=100)
            assert ei.value.status == mpx.ERR_TIMEOUT and time.monotonic() - t0 < 2.0
            with pytest.raises(mpx.MpxError) as ei:
                h.c.host_xfer(PP, group, 1, 0, 3, n, timeout_ms=100)
            assert ei.value.status == mpx.ERR_STATE
        finally:
            h.close()
    h = links(n)
    out = run_ok(h, n, PP, 1, n, 3, check=True)
    assert_call(h, out, PP, 1, n, 3, True)


def test_refusals_on_a_live_context():
    """the statuses of include/mpx_hostlink.h, each decided before any GPU work or wait"""
    n = 4161
    h = links(n)
    c, (tx, rx) = h.c, h.gpu[0]

    def status(fn, *a, **kw):
        with pytest.raises(mpx.MpxError) as ei:
            fn(*a, **kw)
        return ei.value.status

    assert status(c.xfer_hostlink, mpx.MODE_NONBLOCKING, 1, 0, 1, 1, tx, rx, 8) == mpx.ERR_UNSUPPORTED
    assert status(c.host_xfer, mpx.MODE_NONBLOCKING, 0, 1, 0, 1, 8) == mpx.ERR_UNSUPPORTED
    assert status(c.xfer_hostlink, PP, 1, 0, 0, 1, tx, rx, 8) == mpx.ERR_INVALID           # host_rank is a GPU rank
    assert status(c.xfer_hostlink, PP, 1, 1, 1, 1, tx, rx, 8) == mpx.ERR_INVALID           # my_rank is a host endpoint
    assert status(c.host_xfer, PP, 0, 0, 0, 1, 8) == mpx.ERR_INVALID
    assert status(c.xfer_hostlink, PP, 1, 0, 1, 1, rx, tx, 8) == mpx.ERR_INVALID           # not the attached buffers
    assert status(c.xfer_hostlink, PP, 1, 0, 1, 1, tx, rx, h.cap + 1) == mpx.ERR_INVALID
    assert status(c.host_xfer, PP, 0, 1, 0, 1, h.cap + 1) == mpx.ERR_INVALID
    assert status(c.xfer_hostlink, PP, 1, 0, 1, 1, tx, rx, 8, nwg=257) == mpx.ERR_INVALID
    L = c.L
    import ctypes as C
    t = mpx.Timing()
    for flag in (mpx.XFER_STREAM, mpx.XFER_PULL, mpx.XFER_FAN_LL):
        o = mpx.XferOpts(flags=flag)
        assert L.mpx_xfer_hostlink(c.h, PP, 1, 0, 1, 1, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), 8, C.byref(o),
                                   C.byref(t)) == mpx.ERR_INVALID
        assert L.mpx_host_xfer(c.h, PP, 0, 1, 0, 1, 8, C.byref(o), C.byref(t)) == mpx.ERR_INVALID
    # a host endpoint is neither local nor imported: the other entry points refuse it as an unattached rank
    assert status(c.xfer, PP, 1, 0, 1, 1, tx, rx, 8) == mpx.ERR_STATE
    assert status(c.export, 1) == mpx.ERR_STATE
    assert status(c.lat_enable, 1) == mpx.ERR_STATE
    assert status(c.host_attach, 1, 64) == mpx.ERR_STATE and status(c.host_attach, 0, 64) == mpx.ERR_STATE
    assert status(c.attach, 1, 0, tx, rx, 8) == mpx.ERR_STATE
    # an armed GPU rank (armed towards itself: the non-blocking self-pair) refuses a host-link call
    c.arm(mpx.MODE_NONBLOCKING, 1, 0, 0, 1, tx, rx, 8)
    try:
        assert status(c.xfer_hostlink, PP, 1, 0, 1, 1, tx, rx, 8) == mpx.ERR_STATE
    finally:
        c.disarm(0)
    # nothing above took a number or moved a byte: the link still works
    out = run_ok(h, n, UNI, 1, n, 3, check=True)
    assert_call(h, out, UNI, 1, n, 3, True)
    # SDMA and RCCL contexts have no host link
    for engine in ("sdma", "rccl"):
        with mpx.Context(2, engine) as c2:
            assert status(c2.host_attach, 1, 64) == mpx.ERR_UNSUPPORTED
            assert L.mpx_host_xfer(c2.h, PP, 0, 1, 0, 1, 8, None, C.byref(t)) == mpx.ERR_UNSUPPORTED
            assert L.mpx_xfer_hostlink(c2.h, PP, 1, 0, 1, 1, None, None, 8, None, C.byref(t)) == mpx.ERR_UNSUPPORTED
    # mpx_test_advance_link takes a host endpoint as my_rank (as mpx_link_counters does), with token_by = 0 only
    was = [c.link_counters(0, 1), c.link_counters(1, 0)]
    assert status(c.test_advance_link, 1, 0, 0, 0, 1) == mpx.ERR_INVALID                   # an endpoint has no token
    assert status(c.test_advance_link, 1, 0, 1, 1, 1) == mpx.ERR_INVALID
    assert status(c.test_advance_link, 1, 2, 1, 0, 0) == mpx.ERR_INVALID                   # peer out of range
    assert status(c.test_advance_link, 1, 0, MASK, 0, 0) == mpx.ERR_INVALID                # past 2^64 (tx_seq > 0 by now)
    assert [c.link_counters(0, 1), c.link_counters(1, 0)] == was and was[1]["tx_seq"] > 0
    for a, b in ((0, 1), (1, 0)):                                                          # both ends alike: the link goes on
        c.test_advance_link(a, b, 7, 2, 0)
    now = [c.link_counters(0, 1), c.link_counters(1, 0)]
    for k in (0, 1):
        assert now[k] == dict(tx_seq=was[k]["tx_seq"] + 7, rx_seq=was[k]["rx_seq"] + 7, calls=was[k]["calls"] + 2,
                              token=was[k]["token"]), (k, was[k], now[k])
    out = run_ok(h, n, PP, 0, n, 3, check=True)
    assert_call(h, out, PP, 0, n, 3, True)
    # an endpoint that timed out is refused (MPX_ERR_STATE), as a GPU rank is
    hb = HostLinks(64)
    try:
        assert status(hb.c.host_xfer, PP, 0, 1, 0, 1, 8, timeout_ms=50) == mpx.ERR_TIMEOUT
        assert status(hb.c.test_advance_link, 1, 0, 1, 0, 0) == mpx.ERR_STATE
        assert hb.c.link_counters(1, 0)["tx_seq"] == 0
    finally:
        hb.close()


def test_phases_of_a_hostlink_call():
    """mpx_last_phases works for the GPU side as for a pair call"""
    h = links(4161)
    run_ok(h, 4161, PP, 1, 4161, 9)
    ph = h.c.phases(0)
    assert ph["wall_s"] > 0 and ph["kernel_s"] > 0 and ph["armed"] == 0
    assert 0 < ph["first_iter_s"] <= ph["kernel_s"]


@pytest.mark.parametrize("extra,h", [([], "1"), (["-u", "1"], "2")])
def test_mpx_perf_host_link_runs(tmp_path, extra, h):
    """mpx_perf -H: one GPU rank and its endpoint; one record per recorded run,
    written by the side the pair rule makes the writer (group 1: the GPU rank
    with -H 1, the endpoint with -H 2) from its own timing; every payload
    checked; nothing in stderr but the job id, the two INFO lines and run 0's summary"""
    from test_gpu_host import run
    p, recs, side = run(tmp_path, ["-H", h, "-w", "1", "-f", "@G1", "-n", "1", "-p", "1", "-b", "4161", "-i", "7", "-r", "3",
                                   "-c", "1", "-l", "@LOGS"] + extra, gpus="0")
    assert p.returncode == 0, p.stderr[-600:]
    writer = 0 if h == "1" else 1
    assert len(recs) == 2 and len(side) == 2
    for f in recs:
        assert len(f) == 11 and int(f[7]) == 4161 and int(f[8]) == 7
    for f in side:
        assert int(f[2]) == writer and int(f[6]) == 1 - writer and f[3] == "kernel" and f[13] == "host_bulk"
        assert int(f[15]) == 7 and int(f[16]) == 0 and int(f[18]) == 7 and f[20] == "inline"
    lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
    assert len(lines) == 4 and lines[0].startswith("UUID: ") and lines[3].startswith("[Run#: 0]: Total time: "), lines
    info = re.findall(r"INFO: (\S+), rank (\d+) out of 2 ranks, my_group: (\d), group_size: 1, group_rank: 0, my_peer: (\d)",
                      "\n".join(lines[1:3]))
    assert sorted((int(x[1]), int(x[2]), int(x[3])) for x in info) == [(0, 1 - writer, 1), (1, writer, 0)], lines
